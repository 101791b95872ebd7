"""The brush scores on the GPU: the two kernels of csrc/nb_metrics.hip against the float64 statement of tests/brush_metrics_refs.py
on the cases of the CPU test (strided renders inside a NaN-filled buffer, outputs inside guarded buffers, two runs equal as bytes),
and ``metrics.BrushEvaluator`` on the HIP engine against the statement applied to the very renders its passes produced."""
import numpy as np
import pytest
import torch

import brush_catalogue_cases as bc
import brush_metrics_refs as br
from conftest import load_golden
from brushstroke_engine_amd import _lib, brush_metrics_main, config as cfgmod, encoder as encmod, formats, metrics, painting, weights as wmod
from brush_metrics_refs import _expand, _pooled_f64, check_against_passes, check_image_sums, scores_from_passes

pytestmark = pytest.mark.gpu

CASES = br.cases()
IDS = [c["name"] for c in CASES]
GUARD = 64


@pytest.fixture(scope="module")
def gold():
    return load_golden("brush_metrics.npz")


@pytest.fixture(scope="module")
def eng():
    """The HIP engine of tests/test_hip_brush_catalogue.py::eng (R=128, conv_mode h3) and an evaluator on its calibration drawings."""
    e, g = load_golden("engine_r128.npz"), load_golden("brush_catalogue_r128.npz")
    cfg = cfgmod.style1_config(128)
    sd = wmod.random_state_dict(cfg, seed=0)
    esd = encmod.random_encoder_state_dict(5)
    from brushstroke_engine_amd.networks import Generator
    ops = painting.TileOps(Generator(cfg, sd, conv_mode="h3").to("cuda"), encmod.HipGeometryEncoder(esd))
    with torch.no_grad():
        evaluator = metrics.BrushEvaluator(ops, e["uvs_cal_medium"], seed=br.EVAL_SEED)
    return dict(e=e, g=g, cfg=cfg, sd=sd, esd=esd, ops=ops, lib=bc.FixtureLibrary(g, cfg.z_dim), evaluator=evaluator)


class Guarded:
    """A device buffer of ``numel`` elements between two guards of a sentinel value; ``intact()`` after the launches."""

    def __init__(self, numel, dtype, sentinel, guard=GUARD):
        self.buf = torch.full([numel + 2 * guard], sentinel, dtype=dtype, device="cuda")
        self.view, self.guard, self.sentinel = self.buf[guard:guard + numel], guard, sentinel

    def intact(self):
        return bool((self.buf[:self.guard] == self.sentinel).all()) and bool((self.buf[-self.guard:] == self.sentinel).all())


def _render_layouts(ren):
    """ren [n,4,r,r] on the device as views inside NaN-filled buffers: channels 1..4 of an [n,6,r,r] tensor (sample stride 6 r r,
    first plane r r floats in), and a dense copy that starts one float behind a 16-byte boundary."""
    n, _, r, _ = ren.shape
    big = torch.full([n, 6, r, r], float("nan"), dtype=torch.float32, device="cuda")
    big[:, 1:5] = ren
    yield "channels_1_4", big[:, 1:5]
    flat = torch.full([ren.numel() + 8], float("nan"), dtype=torch.float32, device="cuda")
    assert flat.data_ptr() % 16 == 0
    view = flat[1:1 + ren.numel()].view(n, 4, r, r)
    view.copy_(ren)
    yield "offset1", view


def _launch_masks(geom_dev):
    k, r = geom_dev.shape[0], geom_dev.shape[1]
    blur, mask = Guarded(k * r * r, torch.float32, 777.0), Guarded(k * r * r, torch.uint8, 0xAB)
    n_bg, n_fg = Guarded(k, torch.int32, -5, 4), Guarded(k, torch.int32, -5, 4)
    _lib.check(_lib.lib().nb_eval_masks_f32(geom_dev.data_ptr(), k, r, blur.view.data_ptr(), mask.view.data_ptr(), n_bg.view.data_ptr(),
                                            n_fg.view.data_ptr(), torch.cuda.current_stream().cuda_stream), "eval_masks")
    torch.cuda.synchronize()
    assert blur.intact() and mask.intact() and n_bg.intact() and n_fg.intact()
    return (blur.view.view(k, r, r).cpu().numpy(), mask.view.view(k, r, r).cpu().numpy(), n_bg.view.cpu().numpy(), n_fg.view.cpu().numpy())


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_eval_masks_kernel(eng, c):
    g, _ = _expand(c)
    gd = torch.from_numpy(g).cuda()
    a, b = _launch_masks(gd), _launch_masks(gd)
    br.check_masks(*a, g, c["name"])
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    m = eng["ops"].eval_masks(gd)                                          # the ops route: the same bytes
    assert all(x.tobytes() == y.cpu().numpy().tobytes() for x, y in zip(a, (m.blur, m.mask, m.n_bg, m.n_fg)))
    print(f"{c['name']}: blur max err {np.abs(a[0] - br.blur_twice(g)).max():.3g}")


def _launch_metrics(view, tg, m, c, n, r):
    count = r * r
    sums, alpha, deltas = Guarded(4 * n, torch.float32, 777.0), Guarded(n * count, torch.float32, 777.0), Guarded(n * count, torch.float32, 777.0)
    parts = Guarded(n * _lib.NB_BRUSH_METRICS_PARTS * 4, torch.float32, 777.0)
    _lib.check(_lib.lib().nb_brush_metrics_f32(view.data_ptr(), int(view.stride(0)), tg.data_ptr(), m.geom.data_ptr(), m.mask.data_ptr(),
                                               m.geom.shape[0], r, n, float(c["lab_thresh"]), int(c["ignore"]), sums.view.data_ptr(),
                                               alpha.view.data_ptr(), deltas.view.data_ptr(), parts.view.data_ptr(),
                                               torch.cuda.current_stream().cuda_stream), "brush_metrics")
    torch.cuda.synchronize()
    assert sums.intact() and alpha.intact() and deltas.intact() and parts.intact()
    return sums.view.view(n, 4).cpu().numpy(), alpha.view.view(n, r, r).cpu().numpy(), deltas.view.view(n, r, r).cpu().numpy()


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_brush_metrics_kernel(eng, gold, c):
    """Per pixel within 4 eps_ref of float64, the sums within the metrics' tolerances, the alpha planes copied, nothing outside the
    outputs written, and the same bytes from two runs -- on both the 16-byte and the pixel-by-pixel route."""
    eps, ops = float(gold["eps_ref"]), eng["ops"]
    g, g_n = _expand(c)
    n, r = c["renders"].shape[0], g.shape[1]
    m = ops.eval_masks(torch.from_numpy(g).cuda())
    tg = torch.from_numpy(c["targets"]).cuda()
    d64 = br.deltas_f64(c["targets"], c["renders"], c["ignore"])
    worst = 0.0
    for lname, view in _render_layouts(torch.from_numpy(c["renders"]).cuda()):
        a, b = _launch_metrics(view, tg, m, c, n, r), _launch_metrics(view, tg, m, c, n, r)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)), (c["name"], lname)
        sums, alpha, deltas = a
        assert np.array_equal(alpha, c["renders"][:, 3]), (c["name"], lname)
        err = float(np.abs(deltas - d64).max())
        worst = max(worst, err)
        assert err <= br.KERNEL_EPS_FACTOR * eps, (c["name"], lname, err)
        check_image_sums(sums, c, d64, eps)
        s2, a2 = ops.brush_metrics(view, tg, m, c["lab_thresh"], c["ignore"])       # the ops route, no deltas: the same sums
        assert s2.cpu().numpy().tobytes() == sums.tobytes() and np.array_equal(a2.cpu().numpy().reshape(n, r, r), alpha)
    print(f"{c['name']}: dE max err {worst:.3g} (eps_ref {eps:.3g})")
    # the functions on the device ops: the reference's scalars of the case
    ren, gt = torch.from_numpy(c["renders"]).cuda(), torch.from_numpy(g_n).cuda()
    lab = metrics.compute_lab_metrics(tg, ren, gt, lab_thresh=c["lab_thresh"], ignore_transparency=c["ignore"], ops=ops)
    tr = metrics.compute_transparency_metrics(ren, gt, ops=ops)
    br.check_scores({k: np.array([v]) for k, v in {**lab, **tr}.items()}, _pooled_f64(c, br.KERNEL_EPS_FACTOR * eps), eps, c["name"])


def test_values_outside_the_range_do_not_fault(eng):
    """NaN, infinities and values outside 0..1 give unspecified numbers, and the launches complete."""
    ops = eng["ops"]
    vals = torch.tensor([float("nan"), float("inf"), -float("inf"), -1.0, 2.0, 0.5, 1e30, -1e-30], device="cuda")
    geom = vals[torch.arange(2 * 8 * 8, device="cuda") % 8].view(2, 8, 8).contiguous()
    ren = vals[(torch.arange(3 * 4 * 64, device="cuda") * 3) % 8].view(3, 4, 8, 8).contiguous()
    m = ops.eval_masks(geom)
    sums, alpha = ops.brush_metrics(ren, torch.tensor([[float("nan"), 2.0, -1.0]] * 3, device="cuda"), m)
    torch.cuda.synchronize()
    assert sums.shape == (3, 4) and torch.equal(alpha.view(3, 8, 8).isnan(), ren[:, 3].isnan())


# ---------------------------------------------------------------------------------------------------------------------
# the evaluator on the HIP engine
# ---------------------------------------------------------------------------------------------------------------------
def _keep(seen):
    return lambda u, r, t: seen.append((list(u), r.cpu().numpy(), t.cpu().numpy()))


@pytest.fixture(scope="module")
def runs(eng):
    """The four fixture brushes, two rounds: at batch 10 (two units per pass) with the renders kept, at batch 32 and at batch K."""
    out = {}
    with torch.no_grad():
        for name, batch in (("b10", 10), ("b32", 32), ("bk", 5)):
            seen = []
            out[name] = (eng["evaluator"].evaluate(eng["lib"], rounds=br.EVAL_ROUNDS, batch=batch, on_pass=_keep(seen)), seen)
    return out


def test_evaluator_scores_its_renders(eng, gold, runs):
    eps = float(gold["eps_ref"])
    for name, (scores, seen) in runs.items():
        assert scores.ids == eng["lib"].get_style_ids()
        check_against_passes(scores, seen, eng["e"]["uvs_cal_medium"], br.EVAL_ROUNDS, eps)
        assert np.all(np.isfinite(np.stack(list(scores.as_dict().values())))), name
    assert [len(u) for u, _, _ in runs["b10"][1]] == [2, 2, 2, 2] and [len(u) for u, _, _ in runs["b32"][1]] == [6, 2]
    assert [len(u) for u, _, _ in runs["bk"][1]] == [1] * 8
    stream = gold["color_stream"]                                           # the default colours: the reference's stream, brush-major
    for name, (_, seen) in runs.items():
        got = np.concatenate([t.reshape(-1, 5, 3) for _, _, t in seen])
        assert np.array_equal(got, stream), name


def test_functions_agree_with_the_evaluator(eng, runs):
    """``compute_lab_metrics`` / ``compute_transparency_metrics`` on a pass's renders give the evaluator's per-unit numbers."""
    ops, evaluator = eng["ops"], eng["evaluator"]
    geom = evaluator.masks.geom.unsqueeze(1)
    units, ren, tg = runs["bk"][1][3]
    ren, tg = torch.from_numpy(ren).cuda(), torch.from_numpy(tg).cuda()
    unit = evaluator.score_renders(ren, tg).cpu().numpy()[0]              # (KEYS order)
    lab = metrics.compute_lab_metrics(tg, ren, geom, ops=ops)
    tr = metrics.compute_transparency_metrics(ren, geom, ops=ops)
    np.testing.assert_allclose([tr["BG_CLARITY_MEAN"], lab["LAB_E%"], lab["LAB_L2"]], unit[[0, 2, 3]], rtol=1e-6)
    assert np.float32(tr["FG_OPACITY_MEDIAN"]) == unit[1]
    base = painting.TileOpsBase()                                          # and the torch restatements on the same device tensors
    lab_t = metrics.compute_lab_metrics(tg, ren, geom, ops=base)
    tr_t = metrics.compute_transparency_metrics(ren, geom, ops=base)
    np.testing.assert_allclose([tr_t["BG_CLARITY_MEAN"], lab_t["LAB_E%"], lab_t["LAB_L2"]], unit[[0, 2, 3]], rtol=1e-4, atol=1e-4)
    assert np.float32(tr_t["FG_OPACITY_MEDIAN"]) == unit[1]


def test_batch_sizes_agree(gold, runs):
    """batch 32 against batch K.  The scores of each run are held to float64 on its own renders (above); between the runs the renders
    themselves differ by the generator's batch dependence, and the scores by no more than the metrics' tolerances."""
    eps = float(gold["eps_ref"])
    a, b = runs["b32"][0].as_dict(), runs["bk"][0].as_dict()
    for key in metrics.KEYS:
        print(key, np.abs(a[key].astype(np.float64) - b[key]).max(), a[key])
    tol = br.KERNEL_EPS_FACTOR * eps
    assert np.all(np.abs(a["LAB_L2"] - b["LAB_L2"]) <= tol + 1e-5 * np.abs(a["LAB_L2"]))
    assert np.all(np.abs(a["BG_CLARITY_MEAN"] - b["BG_CLARITY_MEAN"]) <= br.CLARITY_TOL)
    ra = np.concatenate([r for _, r, _ in runs["b32"][1]]).astype(np.float64)
    rb = np.concatenate([r for _, r, _ in runs["bk"][1]])
    dr = float(np.abs(ra - rb).max())
    print("renders differ by", dr)
    assert np.all(np.abs(a["FG_OPACITY_MEDIAN"] - b["FG_OPACITY_MEDIAN"]) <= dr)           # a median moves no further than its values
    g = br.geom_f32(load_golden("engine_r128.npz")["uvs_cal_medium"])
    ids = len(a["LAB_E%"])
    # LAB_E%: each run lies in its own band around the threshold; the two bands overlap
    wa = scores_from_passes(runs["b32"][1], (g * 255).astype(np.uint8), ids, br.EVAL_ROUNDS, eps)["LAB_E%_band"]
    wb = scores_from_passes(runs["bk"][1], (g * 255).astype(np.uint8), ids, br.EVAL_ROUNDS, eps)["LAB_E%_band"]
    assert np.all(np.maximum(wa[0], wb[0]) <= np.minimum(wa[1], wb[1]) + 1e-5 * wa[1])


def test_target_colours_reach_the_render(eng, runs):
    with torch.no_grad():
        cols = metrics.default_colors(br.EVAL_SEED, 4, br.EVAL_ROUNDS, 5)
        same = eng["evaluator"].evaluate(eng["lib"], rounds=br.EVAL_ROUNDS, batch=10, colors=cols)
        other = eng["evaluator"].evaluate(eng["lib"], rounds=br.EVAL_ROUNDS, batch=10, colors=1 - cols)
    for key in metrics.KEYS:                                                # the same passes: the same bits
        assert same.as_dict()[key].tobytes() == runs["b10"][0].as_dict()[key].tobytes(), key
    # (brushes 1 and w7 of these random weights paint almost only their primary colour: they match ANY picked colour to 1e-3)
    assert np.all(other.lab_l2 != same.lab_l2) and np.all(np.abs(other.lab_l2 - same.lab_l2)[:2] > 1e-2)


def test_evaluator_with_mapper_and_noise_brush(eng, gold):
    """A mapper's factors come from one ``calibrate`` call and clear the background further; a brush with noise buffers renders in a
    pass of its own, with its noise set, and scores its own renders."""
    e, ops, lib = eng["e"], eng["ops"], eng["lib"]
    ids = lib.get_style_ids()
    with torch.no_grad():
        mapper = painting.StyleUVSMapper(ops, e["uvs_cal_medium"], e["uvs_cal_thick"])
        mapped = metrics.BrushEvaluator(ops, e["uvs_cal_medium"], seed=br.EVAL_SEED, uvs_mapper=mapper)
        seen = []
        s = mapped.evaluate(lib, batch=10, on_pass=_keep(seen))
        plain = eng["evaluator"].evaluate(lib, batch=10)
    assert sorted(mapper.sfactors) == sorted(ids)
    check_against_passes(s, seen, e["uvs_cal_medium"], 1, float(gold["eps_ref"]))
    assert np.all(s.bg_clarity_mean >= plain.bg_clarity_mean) and np.any(s.bg_clarity_mean > plain.bg_clarity_mean)

    from brush_noise_refs import fixture_buffers
    bufs = {k: torch.from_numpy(v) for k, v in fixture_buffers(load_golden("engine_brush_noise_r128.npz"), eng["cfg"]).items()}

    class NoisyLibrary:
        """The W+ brush of the fixture with the noise buffers of tests/golden/engine_brush_noise_r128.npz, between two z brushes."""
        def get_style_ids(self):
            return [ids[0], "noisy", ids[1]]

        def set_style(self, sid, opts):
            if sid != "noisy":
                return lib.set_style(sid, opts)
            opts.set_style_w(torch.from_numpy(eng["g"]["w_brush_ws"]), "noisy", custom_args={"noise_buffers": bufs})
    seen, plain_w = [], []
    cols = metrics.default_colors(br.EVAL_SEED, 3, 1, 5)
    with torch.no_grad():
        s = eng["evaluator"].evaluate(NoisyLibrary(), batch=32, on_pass=_keep(seen))
        eng["evaluator"].evaluate(lib, style_ids=[ids[3]], batch=32, colors=cols[1:2], on_pass=_keep(plain_w))
    assert [[b for b, _ in u] for u, _, _ in seen] == [[0], [1], [2]]
    check_against_passes(s, seen, e["uvs_cal_medium"], 1, float(gold["eps_ref"]))
    assert np.array_equal(seen[1][2], plain_w[0][2]) and np.abs(seen[1][1] - plain_w[0][1]).max() > 1e-3     # the noise set reached the render


def test_main_writes_the_reference_files(eng, gold, tmp_path):
    snap, drawings = str(tmp_path / "engine.npz"), str(tmp_path / "drawings.npz")
    formats.save_engine_snapshot(snap, eng["cfg"], eng["sd"], eng["esd"], preproc_type=None)
    np.savez(drawings, drawings=eng["e"]["uvs_cal_medium"])
    out = tmp_path / "scores"
    style, summary, info = brush_metrics_main.main(["--gan_checkpoint", snap, "--library", "594,0,1", "--drawings", drawings, "--output_dir",
                                                    str(out), "--conv_mode", "h3", "--rounds", "2", "--batch", "10", "--prefix", "t_"])
    rows = open(style).read().splitlines(keepends=True)
    assert rows[0] == str(gold["file_style_header"]) and [r.split()[0] for r in rows[1:]] == ["0", "1", "594"]
    top = open(summary).read().splitlines(keepends=True)
    assert top[0] == str(gold["file_summary_header"]) and len(top) == 2 and len(top[1].split()) == 4
    assert all(len(r) == len(rows[0]) for r in rows) and len(top[1]) == len(top[0])       # every cell right-aligned under its key
    import json
    back = json.load(open(info))
    assert back["ids"] == ["0", "1", "594"]                                # (a seed library lists its ids sorted as strings)
    # the same brushes, seed and rounds through the evaluator of the fixture engine: the same numbers
    with torch.no_grad():
        s = eng["evaluator"].evaluate(eng["lib"], style_ids=["0", "1", "594"], rounds=2, batch=10)
    for key in metrics.KEYS:
        assert np.array_equal(np.array(back["metrics"][key], np.float32), s.as_dict()[key]), key
