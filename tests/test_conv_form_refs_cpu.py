"""CPU check of tests/conv_form_refs.py: from the float64 reference alone, every case that tests/test_hip_conv_forms_f64.py runs
(1) has pre-activations of both signs and |act| on both sides of CLAMP inside EVERY workgroup's block of outputs (every sample,
tile row, tile column and c_out slice of the form under test), so each workgroup's epilogue meets kink and clamp, and (2) tells
a subtly wrong kernel from a right one: each mutation of the reference -- one input channel zeroed, the output shifted by one
pixel row inside a tile, clamp omitted, clamp applied before the gain, the wrong noise form, the last ragged c_out group zeroed
-- moves it by at least CATCH = 20 times the loosest bound any test of that case asserts (and, for the cases with a fused ToRGB,
moves the logits by 20 times their bound).  These are conditions on the seeded inputs, not measurements of a kernel."""
import pytest

import conv_form_refs as cf


def _loosest(d, r, co, fmts, handoff):
    """The loosest bound on the conv output any test of the case asserts: fp32 route and decoded hand-off, over the case's formats."""
    b = max(cf.tol_f32(f, r["scale"]) for f in fmts)
    if handoff:
        want = cf.handoff_want(d, r["ref"], co)
        b = max(b, max(cf.tol_handoff(min(f, 1), r["scale"], d, want, co) for f in fmts))
    return b


def _check(up, n, ci, co, h, w, noise, th, tw, cs, fmts, spt=1, handoff=True, torgb_shape=None):
    d = cf.inputs(up, n, ci, co, h, w)
    r = cf.reference(up, n, ci, co, h, w, noise)
    bad = cf.blocks_meet_kink_and_clamp(r["pre"], r["act"], th, tw, cs, spt)
    assert not bad, f"blocks (sample, channel, row, column) that miss the kink or the clamp: {bad[:8]} ({len(bad)})"
    bound = _loosest(d, r, co, fmts, handoff)
    tg = None
    if torgb_shape:
        tol_conv = max(cf.tol_f32(f, r["scale"]) for f in fmts)
        tg = cf.torgb_reference(d, r["ref"], co, torgb_shape, tol_conv)[0]["logits"]
    for name, m in cf.mutations(up, n, ci, co, h, w, noise, th).items():
        moved = float((m - r["ref"]).abs().max())
        assert moved >= cf.CATCH * bound, f"{name}: moves the reference by {moved:.3e}, bound {bound:.3e}"
        if tg is not None and name != "clamp before the gain":
            # (the logits see the clamped activations: `clamp before the gain` moves them like any other change of ref, but a ToRGB
            #  clamp of 0.5 can hide most of it; the conv output above already catches it)
            lm = cf.torgb_reference(d, m, co, torgb_shape, 0.0)[0]["logits"][0]
            moved = float((lm - tg[0]).abs().max())
            assert moved >= cf.CATCH * float(tg[1].max()), f"{name}: moves the logits by {moved:.3e}, bound {float(tg[1].max()):.3e}"


def _up1_params():
    """(shape, noise, tile rows, c_out per workgroup, formats): the distinct blocks of the up = 1 case table."""
    seen = {}
    for form, shape, route in cf.up1_cases():
        noise = {"f32-shared": "shared", "f32-null": "null"}.get(route, "per")
        th, cs = cf.up1_tile(form, cf.UP1_SHAPES[shape][2])
        seen.setdefault((shape, noise, th, cs), set()).add(cf.UP1_FORMS[form]["fmt"])
    return [k + (tuple(sorted(v)),) for k, v in sorted(seen.items())]


@pytest.mark.parametrize("shape,noise,th,cs,fmts", _up1_params(), ids=lambda v: "".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_up1_cases_meet_kink_and_clamp_and_catch_mutations(shape, noise, th, cs, fmts):
    n, ci, co, h, w = cf.UP1_SHAPES[shape]
    _check(1, n, ci, co, h, w, noise, th, 32, cs, fmts, handoff=co % 8 == 0, torgb_shape=shape if shape in cf.TORGB_SETTINGS else None)


def _up2_params():
    seen = {}
    for form, fmt, ci, co, h, w, n, route in cf.up2_cases():
        seen.setdefault((ci, co, h, w, n) + tuple(cf.up2_tile(form)), set()).add(fmt)
    return [k + (tuple(sorted(v)),) for k, v in sorted(seen.items())]


@pytest.mark.parametrize("ci,co,h,w,n,tqh,tqw,fmts", _up2_params())
def test_up2_cases_meet_kink_and_clamp_and_catch_mutations(ci, co, h, w, n, tqh, tqw, fmts):
    _check(2, n, ci, co, h, w, "per", 2 * tqh, 2 * tqw, 32, fmts)


def _small_params():
    seen = set()
    for up, n, c1, c2, co, h, waves, blocks, noise in cf.small_cases():
        seen.add((up, n, c1 + c2, co, h, noise))
    return sorted(seen)


@pytest.mark.parametrize("up,n,ci,co,h,noise", _small_params())
def test_small_cases_meet_kink_and_clamp_and_catch_mutations(up, n, ci, co, h, noise):
    """(bound: the flat 5e-5 the measured constant SMALL_B may not exceed)"""
    th, tw, spt = cf.small_tile(up, h)
    d = cf.inputs(up, n, ci, co, h, h)
    r = cf.reference(up, n, ci, co, h, h, noise)
    bad = cf.blocks_meet_kink_and_clamp(r["pre"], r["act"], th, tw, 32, spt)
    assert not bad, f"blocks that miss the kink or the clamp: {bad[:8]} ({len(bad)})"
    assert cf.SMALL_B <= cf.SMALL_FLAT
    for name, m in cf.mutations(up, n, ci, co, h, h, noise, th).items():
        moved = float((m - r["ref"]).abs().max())
        assert moved >= cf.CATCH * cf.SMALL_FLAT * r["scale"], f"{name}: moves the reference by {moved:.3e}"


def test_tables_name_every_form():
    """Every up = 1 instantiation the hooks reach (MW 1 / 2 x rows 1 / 2 x round-3 / pipelined / ping-pong x H2 / f8 / f6 x
    persistent or not, and h3s), every older up = 2 form and both small-kernel entries are in the tables, each with its routes."""
    got = {}
    for form, shape, route in cf.up1_cases():
        f = cf.UP1_FORMS[form]
        mw = 2 if cf.UP1_SHAPES[shape][2] > 64 else 1
        got.setdefault((f["fmt"], f["rows"], f["v2"], f["pp"], f["persist"], f["small"], mw), set()).add(route.split("-")[0])
    for fmt, loops in ((0, [(0, 0), (1, 0)]), (1, [(0, 0), (1, 0), (1, 1)]), (2, [(1, 0)])):
        for v2, pp in loops:
            for rows in ((2,) if pp else (1, 2)):
                for persist in ((0, 1) if rows == 2 else (0,)):             # (half-height launches have nothing to walk)
                    for mw in (1, 2):
                        assert got.get((fmt, rows, v2, pp, persist, 0, mw), set()) >= {"f32", "handoff", "torgb"}, (fmt, rows, v2, pp, persist, mw)
    assert got[(0, 2, 1, 0, 0, 1, 1)] >= {"f32", "handoff", "torgb"} and got[(0, 2, 1, 0, 0, 1, 2)] >= {"f32", "handoff"}
    up2 = {(c[0], c[1], c[-1]) for c in cf.up2_cases()}
    for form in ("t12", "t8", "t5", "w16", "w8"):
        for fmt in (0, 1):
            assert {(form, fmt, "f32"), (form, fmt, "handoff")} <= up2
    assert {("pair", 0, "f32"), ("pair", 0, "handoff")} <= up2
    sm = cf.small_cases()
    for up in (1, 2):
        assert {(c[5], c[6]) for c in sm if c[0] == up} >= {(h, wv) for h in (4, 8, 16, 64) for wv in (4, 8)}
        assert {c[8] for c in sm if c[0] == up} == {"per", "shared", "null"} and any(c[7] == 2 for c in sm if c[0] == up)
    assert any(c[0] == 2 and c[3] for c in sm)
