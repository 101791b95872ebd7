"""CPU check of tests/enc_refs.py: from the float64 references alone, (1) conv_ref agrees with the oracle's encoder layer and
upsample_ref with torch's float64 bilinear, (2) every case that tests/test_hip_enc_routes_f64.py runs has pre-activations of both
signs inside EVERY workgroup's block of outputs and, where the output is scaled, scales of both signs for every sample, (3) each
mutation of the reference -- replicate padding, the stride-2 window from 2i, the scale before the LeakyReLU, the scale rows read
with the wrong stride, a later c_out slice with the first slice's bias, the last chunk dropped, a ragged chunk's padding channels
non-zero, the stem's taps transposed, its preprocessing swapped, the bilinear with align_corners=False or with h and w swapped --
moves it by at least CATCH = 20 times the loosest bound any test of that case asserts, and (4) the tables reach all 16
<STRIDE, LW, OUT, F8> instantiations of the large-tile kernel, both hand-off epilogues and every route.  These are conditions on
the seeded inputs and the tables, not measurements of a kernel."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import enc_refs as er


def test_conv_ref_agrees_with_the_oracle_layer():
    """One seeded layer (128 -> 256, stride 2, the encoder's second stage) through the oracle's conv / BatchNorm / LeakyReLU in fp32 and
    through conv_ref on the folded weights.  Bound: the fp32 oracle's own rounding.  K = 9 c_in + 8 operations lie behind an output (the
    sum's terms, each with its folded weight's rounding, the bias, BatchNorm, LeakyReLU); their worst case is K u (sum |x| |w'| + |b'|),
    u = 2^-24, about 1e-3 here and blind to anything finer, so the probabilistic form of that bound is asserted: sqrt(K) u (sum |x| |w'| +
    |b'|) elementwise (rounding errors of both signs add like a random walk), 34 u instead of 1160 u.  The observed ratio is printed
    (observed: 0.023 of the bound, 0.78 u of the magnitude sum, max error 1.8e-6)."""
    from brushstroke_engine_amd import encoder as encmod
    from oracle import painting_oracle as po
    esd = encmod.random_encoder_state_dict(3)
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in esd.items()}
    x = torch.from_numpy(np.random.RandomState(1).randn(2, 128, 16, 24).astype(np.float32))
    want = po._conv_bn_lrelu(x, sd, "encoder.model.2", 2, 1).double()
    w, b = encmod._fold_bn(esd, "encoder.model.2")
    w, b = torch.from_numpy(w), torch.from_numpy(b)
    lin, got = er.conv_ref(x, w, b, 2, 0.01)
    mag = F.conv2d(F.pad(x.double().abs(), (1, 1, 1, 1), mode="reflect"), w.double().abs(), stride=2) + b.double().abs()[None, :, None, None]
    tol = (9 * 128 + 8) ** 0.5 * 2.0 ** -24 * mag
    assert got.shape == want.shape and lin.shape == want.shape
    err = (got - want).abs()
    print(f"[enc-refs] conv_ref vs the fp32 oracle layer: max err {float(err.max()):.3e}, err / bound {float((err / tol).max()):.3f}, "
          f"err / (u x magnitude sum) {float((err / (2.0 ** -24 * mag)).max()):.3f}")
    assert bool((err <= tol).all()), float((err / tol).max())
    # the bound is fine enough to see a BatchNorm fold that is slightly off (eps 1e-3 for 1e-5)
    s_off = torch.from_numpy(np.sqrt((esd["encoder.model.2.conv.1.running_var"] + 1e-5) / (esd["encoder.model.2.conv.1.running_var"] + 1e-3)))
    off = er.conv_ref(x, w * s_off[:, None, None, None], b, 2, 0.01)[1]
    assert bool(((off - want).abs() > tol).any())
    assert float((got - want).abs().max()) > 0                   # (two evaluations, not one compared with itself)


@pytest.mark.parametrize("n,c,h,w", sorted({c[:4] for c in er.UPSAMPLE if not c[5]}))
def test_upsample_ref_agrees_with_torch_float64(n, c, h, w):
    """Against F.interpolate(float64, align_corners=True).  The references differ in the sample coordinate alone: fp32 s = (h - 1) /
    (2 h - 1) and f = s o carry one rounding each, |df| <= 2^-23 (h - 1), and 1 - l one more, 2^-25; the blend is piecewise linear
    and continuous in f with slope <= 2 max|x| per axis, so the results differ by at most 2 max|x| (2^-23 (h + w - 2) + 2^-24)."""
    x = er.upsample_input(n, c, h, w)
    got = er.upsample_ref(x)
    want = F.interpolate(x.double(), scale_factor=2, mode="bilinear", align_corners=True)
    tol = 2 * float(x.abs().max()) * (2.0 ** -23 * (h + w - 2) + 2.0 ** -24)
    assert got.shape == want.shape and float((got - want).abs().max()) <= tol, (float((got - want).abs().max()), tol)
    # the sampled form is the same function
    ns, oys, oxs = er.upsample_sample_points(n, h, w)
    assert torch.equal(er.upsample_ref_at(x, ns, oys, oxs), got[ns, :, oys, oxs])


def _loosest(in_fmt, routes, lin, d, co, b):
    """The loosest bound any test of a conv shape asserts on the (decoded) output, over its routes."""
    out = 0.0
    for r in routes:
        osc = er.oscale_of(d, co) if er.ROUTES[r][2] else None
        out = max(out, er.tol_route(in_fmt, r, lin, er.finish(lin, b, er.SLOPE, osc), osc))
    return out


def _catches(muts, want, bound, what):
    for name, m in muts.items():
        moved = float((m - want).abs().max())
        assert moved >= er.CATCH * bound, f"{what}, {name}: moves the reference by {moved:.3e}, bound {bound:.3e}"


@pytest.mark.parametrize("row", er.LARGE, ids=lambda r: "-".join(map(str, r[:5])) + f"-{r[5][0]}x{r[5][1]}")
def test_large_cases_meet_the_kink_and_catch_mutations(row):
    stride, tile, in_fmt, ci, co, (ho, wo), routes = row
    routes = [r.rstrip("@") for r in routes]
    assert er.launcher_tile(ho, wo) == tile
    d = er.conv_inputs(0, stride, ci, co, ho, wo)
    lin = er.conv_lin(0, stride, ci, co, ho, wo)
    th, tw = er.TILE[tile]
    bad = er.blocks_missing_a_sign(lin + d["b"].double()[None, :, None, None], th, tw, er.CO_WG)
    assert not bad, f"blocks (sample, channel, row, column) whose pre-activations have one sign: {bad[:8]} ({len(bad)})"
    bound = _loosest(in_fmt, routes, lin, d, co, d["b"])
    for scaled in sorted({er.ROUTES[r][2] for r in routes}):
        if scaled:
            osc = er.oscale_of(d, co)
            assert bool(((osc > 0).any(1) & (osc < 0).any(1)).all()), "a sample's output scales have one sign"
            assert float(osc.abs().min()) >= 0.5 and float(osc.abs().max()) <= 1.5 and d["ostride"] > co
        want = er.finish(lin, d["b"], er.SLOPE, er.oscale_of(d, co) if scaled else None)
        muts = er.conv_mutations(0, stride, ci, co, ho, wo, scaled)
        assert "replicate padding" in muts and "last chunk dropped" in muts and ("stride-2 window from 2i" in muts) == (stride == 2)
        assert ("later c_out slices with the first slice's bias" in muts) == (co > 128)
        assert ("ragged chunk's padding channels non-zero" in muts) == (ci % 16 != 0)
        assert ("oscale before the lrelu" in muts and "oscale rows read with stride c_out" in muts) == scaled
        _catches(muts, want, bound, f"{row[:5]} scaled={scaled}")


@pytest.mark.parametrize("shape", sorted({c[:5] for c in er.SMALL}))
def test_small_cases_meet_the_kink_and_catch_mutations(shape):
    stride, ci, co, ho, wo = shape
    routes = [c[5] for c in er.SMALL if c[:5] == shape]
    d = er.conv_inputs(1, stride, ci, co, ho, wo)
    lin = er.conv_lin(1, stride, ci, co, ho, wo)
    th, tw = er.small_tile(wo)
    bad = er.blocks_missing_a_sign(lin + d["b"].double()[None, :, None, None], th, tw, er.SMALL_CO)
    assert not bad, f"blocks whose pre-activations have one sign: {bad[:8]} ({len(bad)})"
    want = er.finish(lin, d["b"])
    muts = er.conv_mutations(1, stride, ci, co, ho, wo, False)
    assert "replicate padding" in muts and "last chunk dropped" in muts and ("stride-2 window from 2i" in muts) == (stride == 2)
    assert ("later c_out slices with the first slice's bias" in muts) == (co > er.SMALL_CO)
    assert "ragged chunk's padding channels non-zero" not in muts and not any(k.startswith("oscale") for k in muts)
    _catches(muts, want, _loosest(0, routes, lin, d, co, d["b"]), str(shape))


@pytest.mark.parametrize("n,h,w,pre", sorted({c[:4] for c in er.STEM}))
def test_stem_cases_meet_the_kink_and_catch_mutations(n, h, w, pre):
    d = er.stem_inputs(n, h, w)
    x = d["x"]
    assert bool((x == 0).any() and (x == 1).any() and ((x > 0) & (x < 1)).any()) and float(x.min()) >= 0 and float(x.max()) <= 1
    lin, want = er.stem_ref(d["x"], d["w"], d["b"], pre)
    bad = er.blocks_missing_a_sign(lin + d["b"].double()[None, :, None, None], 16, 32, 64)
    assert not bad, f"blocks whose pre-activations have one sign: {bad[:8]} ({len(bad)})"
    bound = max(er.tol_decoded(0, f, lin, want, rel=er.STEM_B) for f in (0, 1))
    muts = er.stem_mutations(n, h, w, pre)
    assert ("preprocessing 1 <-> 2" in muts) == (pre != 0) and "taps transposed" in muts
    _catches(muts, want, bound, f"stem {h}x{w} preproc {pre}")


@pytest.mark.parametrize("n,c,h,w", sorted({c[:4] for c in er.UPSAMPLE if not c[5]}))
def test_upsample_cases_catch_mutations(n, c, h, w):
    x = er.upsample_input(n, c, h, w)
    want = er.upsample_ref(x)
    bound = max(er.tol_upsample(x, f, want) for f in {k[4] for k in er.UPSAMPLE if k[:4] == (n, c, h, w)})
    muts = er.upsample_mutations(n, c, h, w)
    assert ("h and w swapped in the scale" in muts) == (h != w)
    _catches(muts, want, bound, f"upsample {n}x{c}x{h}x{w}")


def test_upsample_sampled_case_passes_the_grid_cap_and_catches_mutations():
    """The sampled case: more work items than the capped grid has threads, sample points in the part the strided loop's second pass
    computes, and -- at those sample points, against the bound the GPU test asserts there -- align_corners=False caught (h == w: the
    swapped scale is the same function and does not apply)."""
    (n, c, h, w, fmt, _), = [k for k in er.UPSAMPLE if k[5]]
    assert n * (c // 8) * 4 * h * w > er.UP_GRID_CAP and c % 16 == 0
    ns, oys, oxs = er.upsample_sample_points(n, h, w)
    item = ((ns * (c // 8) + 0) * (2 * h) + oys) * (2 * w) + oxs                    # (channel group 0 of the point)
    assert int((item >= er.UP_GRID_CAP).sum()) > 1000 and int((item < er.UP_GRID_CAP).sum()) > 1000
    assert {(0, 0), (2 * h - 1, 2 * w - 1)} <= set(zip(oys.tolist(), oxs.tolist()))
    x = er.upsample_input(n, c, h, w)
    want = er.upsample_ref_at(x, ns, oys, oxs)
    assert h == w and set(er.upsample_mutations(2, c, 4, 4)) == {"align_corners=False"}
    _catches({"align_corners=False": er.upsample_ref_at(x, ns, oys, oxs, align=False)}, want, er.tol_upsample(x, fmt, want),
             f"upsample {n}x{c}x{h}x{w} at the sample points")


def test_tables_reach_every_instantiation_epilogue_and_route():
    cases = er.large_cases()
    inst = {er.instantiation(s, t, f, r) for s, t, f, ci, co, ho, wo, r, api in cases}
    assert inst == {(s, lw, o, f8) for s in (1, 2) for lw in (4, 5) for o in (0, 1) for f8 in (False, True)}, "16 <STRIDE, LW, OUT, F8>"
    # both hand-off epilogues (32-wide tiles: straight from the accumulators; 16-wide: staged through LDS), each with every
    # H2-container route, each from both operand formats and at both strides
    for tile in ("wide", "narrow"):
        for in_fmt in (0, 1):
            assert {r for s, t, f, ci, co, ho, wo, r, api in cases if t == tile and f == in_fmt} == set(er.ROUTES), (tile, in_fmt)
        for stride in (1, 2):
            got = {r for s, t, f, ci, co, ho, wo, r, api in cases if t == tile and s == stride}
            assert {"win-h2-osc", "win-f8-osc", "f32"} <= got, (tile, stride)
        assert any(api == "handoff" and t == tile and er.ROUTES[r][1] for s, t, f, ci, co, ho, wo, r, api in cases), tile
    assert all(f == 0 for s, t, f, ci, co, ho, wo, r, api in cases if api == "handoff")        # (that entry point takes H2 operands)
    # c_in / c_out edges once per operand format; what each output format can take
    for in_fmt, cis in ((0, {16, 40, 48, 64}), (1, {16, 48, 64})):
        mine = [c for c in cases if c[2] == in_fmt]
        assert {c[3] for c in mine} == cis and {c[4] for c in mine} >= {16, 20, 48, 144}
        assert any(c[4] == 144 and er.ROUTES[c[7]][0] == 1 for c in mine) and any(c[4] == 144 and er.ROUTES[c[7]][0] == 0 for c in mine)
    for s, t, f, ci, co, ho, wo, r, api in cases:
        out_fmt = er.ROUTES[r][0]
        assert out_fmt is None or co % (16 if out_fmt else 8) == 0, (co, r)
        assert f == 0 or ci % 16 == 0
        assert (ho, wo) in (((8, 32), (16, 64)) if t == "wide" else ((16, 16), (32, 48)))
    # small tiles: the sizes, channel counts and routes of the table's comment
    sm = er.SMALL
    assert {(c[0], c[3], c[4]) for c in sm} >= {(1, 4, 4), (2, 4, 4), (1, 8, 8), (1, 16, 16), (2, 8, 32), (1, 6, 8)}
    assert {c[1] for c in sm} == {16, 48, 256} and {c[2] for c in sm} == {8, 40, 64} and {c[5] for c in sm} == {"f32", "h2"}
    assert all(c[5] == "f32" for c in sm if c[2] == 40)
    assert all((c[4] & (c[4] - 1)) == 0 and c[4] >= 4 and c[1] % 16 == 0 for c in sm)
    assert {(c[3], c[4]) for c in er.STEM} == {(p, f) for p in (0, 1, 2) for f in (0, 1)}
    assert {c[1:3] for c in er.STEM} == {(16, 32), (32, 64)}
    assert {c[:5] for c in er.UPSAMPLE} >= {(2, 16, 2, 2, 0), (2, 16, 2, 2, 1), (1, 8, 5, 3, 0), (2, 32, 16, 32, 0), (2, 32, 16, 32, 1)}
