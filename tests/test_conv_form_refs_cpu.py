"""CPU check of tests/conv_form_refs.py: from the float64 reference alone, every case that tests/test_hip_conv_forms_f64.py runs
(1) has pre-activations of both signs and |act| on both sides of CLAMP inside EVERY workgroup's block of outputs (every sample,
tile row, tile column and c_out slice of the form under test), so each workgroup's epilogue meets kink and clamp, and (2) tells
a subtly wrong kernel from a right one: each mutation of the reference -- one input channel zeroed, the output shifted by one
pixel row inside a tile, clamp omitted, clamp applied before the gain, the wrong noise form, the last ragged c_out group zeroed
-- moves it by at least CATCH = 20 times the loosest bound any test of that case asserts (and, for the cases with a fused ToRGB,
moves the logits by 20 times their bound).  The same for the cases of tests/test_hip_up2v_forms_f64.py, with two mutations of their
own -- a persistent workgroup's second item rendered with its first item's channel tables, or with its first item's noise tile --
and the item order of the kernel's tile loop restated.  These are conditions on the seeded inputs, not measurements of a kernel."""
import pytest
import torch

import conv_form_refs as cf


def _loosest(d, r, co, fmts, handoff):
    """The loosest bound on the conv output any test of the case asserts: fp32 route and decoded hand-off, over the case's formats."""
    b = max(cf.tol_f32(f, r["scale"]) for f in fmts)
    if handoff:
        want = cf.handoff_want(d, r["ref"], co)
        b = max(b, max(cf.tol_handoff(min(f, 1), r["scale"], d, want, co) for f in fmts))
    return b


def _check(up, n, ci, co, h, w, noise, th, tw, cs, fmts, spt=1, handoff=True, torgb_shape=None, loosest=_loosest):
    d = cf.inputs(up, n, ci, co, h, w)
    r = cf.reference(up, n, ci, co, h, w, noise)
    bad = cf.blocks_meet_kink_and_clamp(r["pre"], r["act"], th, tw, cs, spt)
    assert not bad, f"blocks (sample, channel, row, column) that miss the kink or the clamp: {bad[:8]} ({len(bad)})"
    bound = loosest(d, r, co, fmts, handoff)
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


# ---------------------------------------------------------------------------------------------------------------------
# the pipelined up = 2 kernel (tests/test_hip_up2v_forms_f64.py)
# ---------------------------------------------------------------------------------------------------------------------

def _up2v_loosest(d, r, co, fmts, handoff):
    """The loosest bound any up2v test of the case asserts: fp32 route and both decoded containers, over the case's operand formats."""
    b = max(cf.tol_f32(f, r["scale"]) for f in fmts)
    if handoff:
        want = cf.handoff_want(d, r["ref"], co)
        b = max(b, max(cf.tol_handoff_x(f, o, r["scale"], d, want, co) for f in fmts for o in (0, 1)))
    return b


def _up2v_params():
    """(shape, noise, tile rows, formats): the distinct blocks of the up2v case tables -- forms, tile loop, in-kernel noise (whose
    own noise image gets test_up2v_noise_case_meets_kink_and_clamp), launcher selection."""
    seen = {}
    for form, fmt, shape, route in cf.up2v_cases() + cf.up2v_loop_cases():
        seen.setdefault((shape, cf.up2v_noise_mode(route), cf.UP2V_FORMS[form][0]), set()).add(fmt)
    for rows in (12, 13):
        seen.setdefault(("N", "per", rows), set()).update((0, 1))
    seen.setdefault(("S12", "per", 12), set()).add(1)
    seen.setdefault(("S13", "per", 13), set()).add(1)
    return [k + (tuple(sorted(v)),) for k, v in sorted(seen.items())]


@pytest.mark.parametrize("shape,noise,rows,fmts", _up2v_params(), ids=lambda v: "".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_up2v_cases_meet_kink_and_clamp_and_catch_mutations(shape, noise, rows, fmts):
    """Tiles of 24 or 26 output rows x 64 columns x 32 channels.  Every workgroup's block meets kink and clamp -- with the hi-only
    reference (operand format 3) as well where that format runs -- and every mutation of mutations() moves the reference by
    >= CATCH x the loosest bound of the case (8e-5 operands into the f8 container where format 2 runs)."""
    n, ci, co, h, w = cf.UP2V_SHAPES[shape]
    _check(2, n, ci, co, h, w, noise, 2 * rows, 64, 32, fmts, handoff=co % 8 == 0, loosest=_up2v_loosest)
    if 3 in fmts:
        r = cf.reference(2, n, ci, co, h, w, noise, hi=True)
        bad = cf.blocks_meet_kink_and_clamp(r["pre"], r["act"], 2 * rows, 64, 32)
        assert not bad, f"hi-only reference: blocks that miss the kink or the clamp: {bad[:8]} ({len(bad)})"


def test_up2v_noise_case_meets_kink_and_clamp():
    """Shape N with the noise the in-kernel case really uses (the oracle's float64 evaluation of conv_form_refs.up2v_noise_case):
    every block of both tile heights on both sides of kink and clamp; the noise is no constant of a sample (its positions differ)."""
    n, ci, co, h, w = UP = cf.UP2V_SHAPES["N"]
    nz = cf.up2v_noise_ref()
    assert nz.shape == (n, 2 * h, 2 * w) and float(nz.std()) > 0.3 and not torch.equal(nz[0], nz[1])
    pre, act, ref = cf.epilogue(cf.linear(2, *UP), cf.inputs(2, *UP), nz)
    for rows in (12, 13):
        assert not cf.blocks_meet_kink_and_clamp(pre, act, 2 * rows, 64, 32), rows
    # a noise tile shifted by one row (the 13-row form writes it behind the K loop) moves the reference by CATCH bounds
    scale = float(cf.linear(2, *UP).abs().max()) * cf.GAIN
    moved = float((cf.epilogue(cf.linear(2, *UP), cf.inputs(2, *UP), torch.roll(nz, 1, dims=1))[2] - ref).abs().max())
    assert moved >= cf.CATCH * cf.tol_f32(1, scale), moved


@pytest.mark.parametrize("shape", ["P1", "P2"])
def test_up2v_tile_loop_items_and_mutations(shape):
    """The item order of tile_coords restated (up2v_item) on a grid of 256: a permutation of the item list; P1 in the renumbered
    order, P2 in the plain one; every workgroup's second item differs from its first in sample, on P2 also in tile row or slice;
    state carried from the first item into the second -- channel tables, noise tile -- moves the reference by CATCH bounds."""
    n, ci, co, h, w = UP = cf.UP2V_SHAPES[shape]
    tiles_x, tiles_y, slices, items_x, items = cf.up2v_geometry(shape, 12)
    grid = cf.UP2V_CUS
    assert grid < items <= 2 * grid
    assert (items % 8 == 0 and grid % 8 == 0) if shape == "P1" else (items % 8 != 0 and items_x % 8 != 0)
    for g in (grid, items):                                        # (persistent; one workgroup per tile)
        got = sorted(cf.up2v_item(l, items, items_x, slices, tiles_x, g) for l in range(items))
        assert got == sorted((a, b, c, e) for a in range(n) for b in range(tiles_y) for c in range(tiles_x) for e in range(slices))
    if shape == "P1":
        assert [cf.up2v_item(l, items, items_x, slices, tiles_x, grid) for l in range(items)] != \
               [cf.up2v_item(l, items + 1, items_x, slices, tiles_x, grid) for l in range(items)]         # (renumbered != plain)
    pairs = cf.up2v_second_items(shape)
    assert len(pairs) == items - grid
    for a, b in pairs:
        assert a[0] != b[0] and (shape == "P1" or a[1] != b[1] or a[3] != b[3]), (a, b)
    d, r = cf.inputs(2, *UP), cf.reference(2, *UP)
    want = cf.handoff_want(d, r["ref"], co)
    b_f32 = max(cf.tol_f32(f, r["scale"]) for f in (0, 1))
    b_out = max(cf.tol_handoff(f, r["scale"], d, want, co) for f in (0, 1))
    for name, (m, mw) in cf.up2v_loop_mutations(shape).items():
        moved, moved_w = float((m - r["ref"]).abs().max()), float((mw - want).abs().max())
        assert moved >= cf.CATCH * b_f32, f"{name}: moves the reference by {moved:.3e}, bound {b_f32:.3e}"
        assert moved_w >= cf.CATCH * b_out, f"{name}: moves the hand-off value by {moved_w:.3e}, bound {b_out:.3e}"
        # ... and inside EVERY later item's block, not in one of them only
        th = 24
        for (_, (n2, y2, x2, s2)) in pairs:
            blk = (m - r["ref"])[n2, 32 * s2:32 * s2 + 32, th * y2:th * y2 + th, 64 * x2:64 * x2 + 64].abs().max()
            assert float(blk) >= cf.CATCH * b_f32, f"{name}: item {(n2, y2, x2, s2)} moves by {float(blk):.3e} only"


def test_up2v_tables_name_every_instantiation():
    """All 36 instantiations of nb_up2v_launch -- 3 forms x operand formats 0 .. 3 x {fp32, H2 container, f8 container} -- are in
    up2v_cases(); B and C occur with all three noise modes at both tile heights; every chunk count (1, 4, 5, 7) in every operand
    format; the tile loop in both 12-row forms, both formats and both orders; the selection shapes select what their names say."""
    cases = cf.up2v_cases()
    inst = {(form, fmt, {"f32": 0, "handoff-h2": 1, "handoff-f8": 2}[route.replace("-shared", "").replace("-null", "")]) for form, fmt, s, route in cases}
    assert inst == {(form, fmt, o) for form in cf.UP2V_FORMS for fmt in range(4) for o in range(3)} and len(inst) == 36
    for s in "BC":
        for rows in (12, 13):
            assert {cf.up2v_noise_mode(r) for form, fmt, s_, r in cases if s_ == s and cf.UP2V_FORMS[form][0] == rows} == {"per", "shared", "null"}
    for form in cf.UP2V_FORMS:
        for fmt in range(4):
            assert {cf.UP2V_SHAPES[s][1] // 16 for f_, m_, s, r in cases if (f_, m_) == (form, fmt)} == {1, 4, 5, 7}
    assert all(r.startswith("f32") for f_, m_, s, r in cases if s == "D") and {s for f_, m_, s, r in cases} == set("ABCD")
    loop = cf.up2v_loop_cases()
    assert {(f_, m_, s, r.split("-")[0]) for f_, m_, s, r in loop} == {(f_, m_, s, r) for f_ in ("r12p", "r12") for m_ in (0, 1) for s in ("P1", "P2")
                                                                    for r in ("f32", "handoff")}
    for s, rows in (("S12", 12), ("S13", 13)):
        n, ci, co, h, w = cf.UP2V_SHAPES[s]
        assert cf.up2v_select(ci, co, n, h, w) == ("modconv3x3_up2v_kernel", rows), s
    assert cf.up2v_select(16, 128, 20, 24, 32)[0] == "modconv3x3_up2_h3_kernel"          # (the shape first proposed for S12)
