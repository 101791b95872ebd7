"""The inputs of the perceptual brush scores on the GPU: the three entries of csrc/nb_metric_patches.hip against the float64 statement of
tests/metric_patches_refs.py on the cases of the CPU test (strided renders inside NaN-filled buffers, outputs inside guarded buffers,
two runs equal as bytes, the ops route equal to the direct call), ``LPIPS.pair_distance`` on the kernels against ``lpips_f64`` of the
very pairs the kernel made, and ``metrics.BrushEvaluator`` with an LPIPS network on the HIP engine against the statement applied to
the renders its passes produced."""
import numpy as np
import pytest
import torch

import brush_catalogue_cases as bc
import brush_metrics_refs as br
import clarity_refs as cr
import lpips_refs as lr
import metric_patches_refs as mp
from conftest import load_golden
from brushstroke_engine_amd import _lib, brush_metrics_main, config as cfgmod, encoder as encmod, formats, metrics, painting, perceptual, tile_ops
from brushstroke_engine_amd import weights as wmod

pytestmark = pytest.mark.gpu

CASES = mp.pair_cases()
IDS = [c["name"] for c in CASES]
GUARD = 64
P_EVAL = 64                                # default_patch_width(128)


@pytest.fixture(scope="module")
def eng():
    """The HIP engine of tests/test_hip_brush_metrics.py::eng (R=128, conv_mode h3, the calibration drawings uvs_cal_medium), built here
    again, and a slim ``alex`` on the kernels."""
    e, g = load_golden("engine_r128.npz"), load_golden("brush_catalogue_r128.npz")
    cfg = cfgmod.style1_config(128)
    sd = wmod.random_state_dict(cfg, seed=0)
    esd = encmod.random_encoder_state_dict(5)
    from brushstroke_engine_amd.networks import Generator
    ops = painting.TileOps(Generator(cfg, sd, conv_mode="h3").to("cuda"), encmod.HipGeometryEncoder(esd))
    with torch.no_grad():
        evaluator = metrics.BrushEvaluator(ops, e["uvs_cal_medium"], seed=br.EVAL_SEED)
    s = lr.SLIM["alex"]
    w = lr.slim_weights("alex", s["channels"], s["seed"], s["size"])
    return dict(e=e, g=g, cfg=cfg, sd=sd, esd=esd, ops=ops, lib=bc.FixtureLibrary(g, cfg.z_dim), evaluator=evaluator, w=w, net=perceptual.LPIPS(w, route="hip"))


class Guarded:
    """A device buffer of ``numel`` elements between two guards of a sentinel value; ``intact()`` after the launches."""

    def __init__(self, numel, dtype, sentinel, guard=GUARD):
        self.buf = torch.full([numel + 2 * guard], sentinel, dtype=dtype, device="cuda")
        self.view, self.guard, self.sentinel = self.buf[guard:guard + numel], guard, sentinel

    def intact(self):
        return bool((self.buf[:self.guard] == self.sentinel).all()) and bool((self.buf[-self.guard:] == self.sentinel).all())


def _render_layouts(ren):
    """ren [n,4,r,r] on the device as views inside NaN-filled buffers: channels 1..4 of an [n,6,r,r] tensor, and a dense copy that
    starts one float behind a 16-byte boundary."""
    n, _, r, _ = ren.shape
    big = torch.full([n, 6, r, r], float("nan"), dtype=torch.float32, device="cuda")
    big[:, 1:5] = ren
    yield "channels_1_4", big[:, 1:5]
    flat = torch.full([ren.numel() + 8], float("nan"), dtype=torch.float32, device="cuda")
    assert flat.data_ptr() % 16 == 0
    view = flat[1:1 + ren.numel()].view(n, 4, r, r)
    view.copy_(ren)
    yield "offset1", view


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _launch_guidance(geom):
    k, r = geom.shape[0], geom.shape[1]
    blur1, n_bg = Guarded(k * r * r, torch.float32, 777.0), Guarded(k, torch.int32, -5, 4)
    _lib.check(_lib.lib().nb_bg_guidance_f32(geom.data_ptr(), k, r, blur1.view.data_ptr(), n_bg.view.data_ptr(), _stream()), "bg_guidance")
    torch.cuda.synchronize()
    assert blur1.intact() and n_bg.intact()
    return blur1.view.view(k, r, r).clone(), n_bg.view.clone()


def _launch_mean(view, blur1, n_bg):
    n, r, k = view.shape[0], view.shape[2], blur1.shape[0]
    parts, mean = Guarded(n * _lib.NB_BG_MEAN_PARTS * 3, torch.float32, 777.0), Guarded(3 * n, torch.float32, 777.0)
    _lib.check(_lib.lib().nb_bg_mean_colors_f32(view.data_ptr(), int(view.stride(0)), blur1.data_ptr(), n_bg.data_ptr(), k, r, n, parts.view.data_ptr(),
                                                mean.view.data_ptr(), _stream()), "bg_mean_colors")
    torch.cuda.synchronize()
    assert parts.intact() and mean.intact()
    return mean.view.view(n, 3).clone()


def _launch_pairs(view, blur1, mean, o0, o1, s1, c):
    n, r, p = view.shape[0], view.shape[2], c["p"]
    out = Guarded(2 * n * 3 * p * p, torch.float32, 777.0)
    flags = (_lib.NB_METRIC_PAIRS_TRANSPOSE if c["transpose"] else 0) | (_lib.NB_METRIC_PAIRS_MASKED if c["masked"] else 0)
    _lib.check(_lib.lib().nb_metric_pairs_f32(view.data_ptr(), int(view.stride(0)), blur1.data_ptr() if c["masked"] else None,
                                              mean.data_ptr() if c["masked"] else None, o0.data_ptr(), o1.data_ptr(), None if s1 is None else s1.data_ptr(),
                                              blur1.shape[0], r, p, n, flags, out.view.data_ptr(), _stream()), "metric_pairs")
    torch.cuda.synchronize()
    assert out.intact()
    return out.view.view(2 * n, 3, p, p).clone()


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_kernels_against_float64(eng, c):
    """The blur within BLUR1_TOL, the counts those of the blur, the means within MEAN_TOL, kept pixels within PIXEL_TOL and filled ones
    within FILL_TOL of float64; nothing outside the outputs written; the same bytes from two runs and from the ops route -- on the
    strided and on the misaligned layout of the renders."""
    ops, ref = eng["ops"], mp.statement(c)
    ren, geom, o0, o1, s1 = mp.to_torch(c, "cuda")
    blur1, n_bg = _launch_guidance(geom)
    again = _launch_guidance(geom)
    g = ops.bg_guidance(geom)
    assert torch.equal(blur1, again[0]) and torch.equal(n_bg, again[1]) and torch.equal(blur1, g.blur1) and torch.equal(n_bg, g.n_bg)
    mp.check_guidance(blur1.cpu().numpy(), n_bg.cpu().numpy(), br.geom_f32(c["geom_u8"]), c["name"])
    worst = [0.0, 0.0]
    for lname, view in _render_layouts(ren):
        what = (c["name"], lname)
        mean = _launch_mean(view, blur1, n_bg)
        assert mean.cpu().numpy().tobytes() == _launch_mean(view, blur1, n_bg).cpu().numpy().tobytes(), what
        assert ops.bg_mean_colors(view, g).cpu().numpy().tobytes() == mean.cpu().numpy().tobytes(), what
        worst[0] = max(worst[0], mp.check_mean(mean.cpu().numpy(), ref, what))
        x = _launch_pairs(view, blur1, mean, o0, o1, s1, c)
        assert x.cpu().numpy().tobytes() == _launch_pairs(view, blur1, mean, o0, o1, s1, c).cpu().numpy().tobytes(), what
        via = ops.metric_pairs(view, g if c["masked"] else None, mean if c["masked"] else None, o0, o1, s1, c["p"], c["transpose"], c["masked"])
        assert via.cpu().numpy().tobytes() == x.cpu().numpy().tobytes(), what
        worst[1] = max(worst[1], mp.check_pairs(x.cpu().numpy(), ref, what))
    print(f"{c['name']}: mean max err {worst[0]:.3g}, pixel max err {worst[1]:.3g}")


def test_plan_values_outside_the_range_are_clamped(eng):
    """Offsets and indices live on the device; the kernel clamps them, so a bad plan reads inside the renders."""
    ops = eng["ops"]
    c = next(x for x in CASES if x["name"] == "r20_n7_k5_p7")
    ren, geom, o0, o1, s1 = mp.to_torch(c, "cuda")
    g = ops.bg_guidance(geom)
    mean = ops.bg_mean_colors(ren, g)
    far0, far1, src = o0.clone(), o1.clone(), s1.clone()
    far0[0], far1[1], src[2] = torch.tensor([-5, 1 << 30], device="cuda"), torch.tensor([99, -(1 << 30)], device="cuda"), 1 << 20
    inside0, inside1, isrc = far0.clamp(0, 13), far1.clamp(0, 13), src.clamp(0, 6)
    a = ops.metric_pairs(ren, g, mean, far0, far1, src, 7)
    b = ops.metric_pairs(ren, g, mean, inside0, inside1, isrc, 7)
    torch.cuda.synchronize()
    assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------------------
# pair_distance on the kernels
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch", sorted(mp.DISTANCE_CASES))
def test_pair_distance_on_kernel_made_pairs(eng, arch):
    """Slim ``alex`` at 64 x 64 and ``vgg`` at 32 x 32 on the pairs the kernel makes from the seeded renders of the distance case,
    against ``lpips_f64`` of the same float32 pairs, within ``bound`` with SPLIT_F16_FACTOR; the pairs keep every ReLU and pool
    decision KINK_MARGIN float32-route errors from zero (a condition of the comparison, asserted); and against the two-image call."""
    ops = eng["ops"]
    c, w = mp.distance_case(arch)
    ren, geom, o0, o1, s1 = mp.to_torch(c, "cuda")
    g = ops.bg_guidance(geom)
    x = ops.metric_pairs(ren, g, ops.bg_mean_colors(ren, g), o0, o1, s1, c["p"], True, True)
    xh = x.cpu().numpy()
    mp.check_pairs(xh, mp.statement(c), arch)
    min_pre, min_gap, err = mp.pair_margins(w, xh)
    print(f"[pair_distance] {arch}: |pre| {min_pre / err:.0f} errors, pool gap {min_gap / err:.0f} errors")
    assert min_pre >= lr.KINK_MARGIN * err and min_gap >= lr.KINK_MARGIN * err
    n = x.shape[0] // 2
    want = mp.distance_f64(w, xh)
    t32 = lr.lpips_f64(w, xh[:n], xh[n:], dtype=torch.float32).numpy()
    tol = lr.SPLIT_F16_FACTOR * float(np.abs(t32.astype(np.float64) - want).max()) + cr.ULP_FLOOR * cr.EPS32 * np.abs(want)
    net = eng["net"] if arch == "alex" else perceptual.LPIPS(w, route="hip")
    calls = net.trunk_calls
    got = net.pair_distance(x)
    assert net.trunk_calls == calls + 1 and got.shape == (n,) and not got.requires_grad
    two = net(x[:n].contiguous(), x[n:].contiguous()).detach()
    torch.cuda.synchronize()
    for name, v in (("pair_distance", got), ("two images", two)):
        e = np.abs(v.cpu().numpy().astype(np.float64) - want)
        print(f"[pair_distance] {arch} {name}: error {e.max():.3g}, float32 torch route {np.abs(t32 - want).max():.3g}, bound {tol.min():.3g}")
        assert np.all(e <= tol), (arch, name, v, want)
    assert torch.equal(net.pair_distance(x), got)
    with pytest.raises(ValueError, match="minimum side"):
        net.pair_distance(x[:, :, :15, :15])


# ---------------------------------------------------------------------------------------------------------------------
# the evaluator on the HIP engine
# ---------------------------------------------------------------------------------------------------------------------
def _keep(seen):
    return lambda u, r, t, own_renders=None: seen.append((list(u), r.cpu().numpy(), own_renders.cpu().numpy()))


def _restated_pairs(c):
    """The float32 torch route of a pair case: the ``TileOpsBase`` restatement on the host."""
    ops = tile_ops.TileOpsBase()
    ren, geom, o0, o1, s1 = mp.to_torch(c)
    g = ops.bg_guidance(geom)
    return ops.metric_pairs(ren, g if c["masked"] else None, ops.bg_mean_colors(ren, g) if c["masked"] else None, o0, o1, s1, c["p"],
                            c["transpose"], c["masked"]).numpy()


def _check_against_passes(scores, seen, eng, n_brushes, rounds, plan):
    """Every perceptual score within SPLIT_F16_FACTOR x the float32 torch route's error (restated pairs, float32 network) plus the ulp
    floor of the float64 statement on the renders the passes produced."""
    w, geom = eng["w"], eng["e"]["uvs_cal_medium"]
    want = mp.scores_from_passes(w, geom, seen, n_brushes, rounds, plan, P_EVAL)
    f32 = lambda x: lr.lpips_f64(w, x[:len(x) // 2], x[len(x) // 2:], dtype=torch.float32).numpy()
    t32 = mp.scores_from_passes(w, geom, seen, n_brushes, rounds, plan, P_EVAL, pairs=_restated_pairs, dist=f32)
    for key in metrics.PERCEPTUAL_KEYS:
        e32 = float(np.abs(t32[key] - want[key]).max())
        tol = lr.SPLIT_F16_FACTOR * e32 + cr.ULP_FLOOR * cr.EPS32 * np.abs(want[key])
        e = np.abs(scores.perceptual[key].astype(np.float64) - want[key])
        print(f"[evaluator] {key}: {scores.perceptual[key]}, error {e.max():.3g}, float32 torch route {e32:.3g}, bound {tol.min():.3g}")
        assert np.all(e <= tol), (key, scores.perceptual[key], want[key])


def test_evaluator_with_lpips(eng):
    """Three brushes, two rounds, slim ``alex``: held to the float64 statement on its own renders with the plan of ``default_crops``;
    a second run gives the same bits; the four existing scores are those of a run without the network, bit for bit."""
    evaluator, lib, net = eng["evaluator"], eng["lib"], eng["net"]
    ids = lib.get_style_ids()[:3]
    seen = []
    with torch.no_grad():
        s = evaluator.evaluate(lib, style_ids=ids, rounds=2, batch=10, lpips=net, on_pass=_keep(seen))
        again = evaluator.evaluate(lib, style_ids=ids, rounds=2, batch=10, lpips=net)
        plain = evaluator.evaluate(lib, style_ids=ids, rounds=2, batch=10)
    assert [u for u, _, _ in seen] == [[(0, 0), (0, 1)], [(1, 0), (1, 1)], [(2, 0), (2, 1)]]
    assert all(r.shape == (10, 4, 128, 128) and o.shape == r.shape and not np.array_equal(r, o) for _, r, o in seen)
    assert s.keys() == metrics.KEYS + metrics.PERCEPTUAL_KEYS and plain.perceptual is None
    for key in s.keys():
        assert s.as_dict()[key].tobytes() == again.as_dict()[key].tobytes(), key
    for key in metrics.KEYS:
        assert s.as_dict()[key].tobytes() == plain.as_dict()[key].tobytes(), key
    assert np.all(np.isfinite(np.stack([s.perceptual[k] for k in metrics.PERCEPTUAL_KEYS]))) and all(np.all(s.perceptual[k] > 0) for k in metrics.PERCEPTUAL_KEYS)
    und = mp.guidance_f64(br.geom_f32(eng["e"]["uvs_cal_medium"]))[3]
    assert not und.any()                                                    # (the smallest gap to 0.99 is 4e-3)
    _check_against_passes(s, seen, eng, 3, 2, metrics.default_crops(br.EVAL_SEED, 3, 2, 5, 128, P_EVAL))


def test_evaluator_with_lpips_and_noise_brush(eng):
    """A brush with noise buffers goes through passes of its own, both renders with its noise set, and scores its own renders."""
    lib, cfg = eng["lib"], eng["cfg"]
    ids = lib.get_style_ids()
    from brush_noise_refs import fixture_buffers
    bufs = {k: torch.from_numpy(v) for k, v in fixture_buffers(load_golden("engine_brush_noise_r128.npz"), cfg).items()}

    class NoisyLibrary:
        def get_style_ids(self):
            return [ids[0], "noisy"]

        def set_style(self, sid, opts):
            if sid != "noisy":
                return lib.set_style(sid, opts)
            opts.set_style_w(torch.from_numpy(eng["g"]["w_brush_ws"]), "noisy", custom_args={"noise_buffers": bufs})
    seen, plain = [], []
    with torch.no_grad():
        s = eng["evaluator"].evaluate(NoisyLibrary(), batch=32, lpips=eng["net"], on_pass=_keep(seen))
        eng["evaluator"].evaluate(lib, style_ids=[ids[3]], batch=32, lpips=eng["net"], on_pass=_keep(plain))
    assert [[b for b, _ in u] for u, _, _ in seen] == [[0], [1]]
    assert np.abs(seen[1][2] - plain[0][2]).max() > 1e-3                    # the noise set reached the second render too
    _check_against_passes(s, seen, eng, 2, 1, metrics.default_crops(br.EVAL_SEED, 2, 1, 5, 128, P_EVAL))


def test_main_writes_seven_columns_with_lpips_weights(eng, tmp_path):
    """``brush_metrics_main --lpips_weights``: the two text files with the seven sorted columns in the reference's format, and the
    numbers of the evaluator with the same network, seed and default plan."""
    import json
    snap, drawings, wpath = str(tmp_path / "engine.npz"), str(tmp_path / "drawings.npz"), str(tmp_path / "alex_slim.npz")
    formats.save_engine_snapshot(snap, eng["cfg"], eng["sd"], eng["esd"], preproc_type=None)
    np.savez(drawings, drawings=eng["e"]["uvs_cal_medium"])
    np.savez(wpath, **eng["w"])
    style, summary, info = brush_metrics_main.main(["--gan_checkpoint", snap, "--library", "594,0", "--drawings", drawings, "--output_dir",
                                                    str(tmp_path / "scores"), "--conv_mode", "h3", "--batch", "10", "--lpips_weights", wpath])
    keys = list(metrics.KEYS + metrics.PERCEPTUAL_KEYS)
    rows = open(style).read().splitlines(keepends=True)
    assert rows[0] == "SEED            " + metrics.file_line(keys) and [r.split()[0] for r in rows[1:]] == ["0", "594"]
    assert all(len(r) == len(rows[0]) and len(r.split()) == 8 for r in rows)
    top = open(summary).read().splitlines(keepends=True)
    assert top[0] == metrics.file_line(keys) and len(top) == 2 and len(top[1].split()) == 7 and len(top[1]) == len(top[0])
    back = json.load(open(info))
    assert back["ids"] == ["0", "594"] and list(back["metrics"]) == keys
    with torch.no_grad():
        s = eng["evaluator"].evaluate(eng["lib"], style_ids=["0", "594"], batch=10, lpips=eng["net"])
    for key in keys:
        assert np.array_equal(np.array(back["metrics"][key], np.float32), s.as_dict()[key]), key
