"""The stitching scores on the GPU: the two entries of csrc/nb_stitch_metrics.hip against the numpy statement of tests/stitch_refs.py on
the cases of the CPU test (images as strided views inside NaN-filled buffers and one float behind a 16-byte boundary, outputs inside
guarded buffers, two runs equal as bytes, the ops route equal to the direct call), ``LPIPS.pair_distance`` on the pairs the kernel makes
against ``lpips_f64`` of the same pairs, and ``metrics.BrushEvaluator`` with a ``StitchSetup`` on the HIP engine against the statement
applied to the images its passes rendered."""
import json

import numpy as np
import pytest
import torch

import brush_catalogue_cases as bc
import brush_metrics_refs as br
import clarity_refs as cr
import lpips_refs as lr
import metric_patches_refs as mp
import stitch_refs as sr
from conftest import load_golden
from brushstroke_engine_amd import _lib, brush_metrics_main, config as cfgmod, encoder as encmod, formats, metrics, painting, perceptual
from brushstroke_engine_amd import weights as wmod

pytestmark = pytest.mark.gpu

CASES = sr.pair_cases()
IDS = [c["name"] for c in CASES]
CROPS = sr.crop_cases()
GUARD = 64
D_FULL, KS, MARGIN, MIN_OVERLAP = 192, 3, 10, 50


@pytest.fixture(scope="module")
def eng():
    """The HIP engine of tests/test_hip_metric_patches.py::eng (R=128, conv_mode h3, the calibration drawings uvs_cal_medium), built here
    again, a slim ``alex`` on the kernels, and KS of the drawings padded to D_FULL x D_FULL as full-size drawings."""
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
    full = np.full((KS, D_FULL, D_FULL), 255, np.uint8)
    full[:, 24:152, 40:168] = e["uvs_cal_medium"][:KS]
    return dict(e=e, g=g, cfg=cfg, sd=sd, esd=esd, ops=ops, lib=bc.FixtureLibrary(g, cfg.z_dim), evaluator=evaluator, w=w,
                net=perceptual.LPIPS(w, route="hip"), full=full)


class Guarded:
    """A device buffer of ``numel`` elements between two guards of a sentinel value; ``intact()`` after the launches.  An odd guard
    puts a float view off the 16-byte boundary."""

    def __init__(self, numel, dtype, sentinel, guard=GUARD):
        self.buf = torch.full([numel + 2 * guard], sentinel, dtype=dtype, device="cuda")
        self.view, self.guard, self.sentinel = self.buf[guard:guard + numel], guard, sentinel

    def intact(self):
        return bool((self.buf[:self.guard] == self.sentinel).all()) and bool((self.buf[-self.guard:] == self.sentinel).all())


def _fake_layouts(fake):
    """fake [2n,3,r,r] on the device as views inside NaN-filled buffers: channels 1..3 of a [2n,5,r,r] tensor, and a dense copy that
    starts one float behind a 16-byte boundary."""
    n2, _, r, _ = fake.shape
    big = torch.full([n2, 5, r, r], float("nan"), dtype=torch.float32, device="cuda")
    big[:, 1:4] = fake
    yield "channels_1_3", big[:, 1:4]
    flat = torch.full([fake.numel() + 8], float("nan"), dtype=torch.float32, device="cuda")
    assert flat.data_ptr() % 16 == 0
    view = flat[1:1 + fake.numel()].view(n2, 3, r, r)
    view.copy_(fake)
    yield "offset1", view


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _launch_pairs(view, ra, rb, margin, guard=GUARD):
    n, r = view.shape[0] // 2, view.shape[2]
    s = r - 3 * margin
    out, l1 = Guarded(4 * n * 3 * s * s, torch.float32, 777.0, guard), Guarded(2 * n, torch.float32, 777.0)
    parts = Guarded(n * _lib.NB_STITCH_PARTS * 2, torch.float32, 777.0)
    _lib.check(_lib.lib().nb_stitch_pairs_f32(view.data_ptr(), int(view.stride(0)), ra.data_ptr(), rb.data_ptr(), n, r, margin, out.view.data_ptr(),
                                              l1.view.data_ptr(), parts.view.data_ptr(), _stream()), "stitch_pairs")
    torch.cuda.synchronize()
    assert out.intact() and l1.intact() and parts.intact()
    return out.view.view(4 * n, 3, s, s).clone(), l1.view.clone()


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_pairs_kernel_against_the_statement(eng, c):
    """The pair buffer equal to the statement as bytes and every sum within ``l1_bound`` of float64, on the strided and on the misaligned
    layout of the images and with the output on and off a 16-byte boundary; nothing outside the outputs written; the same bytes from
    two runs and from the ops route."""
    ops = eng["ops"]
    fake, ra, rb = sr.to_torch(c, "cuda")
    worst = 0.0
    for lname, view in _fake_layouts(fake):
        for guard in (GUARD, GUARD - 1):
            what = (lname, guard)
            x, l1 = _launch_pairs(view, ra, rb, c["margin"], guard)
            x2, l12 = _launch_pairs(view, ra, rb, c["margin"], guard)
            assert x.cpu().numpy().tobytes() == x2.cpu().numpy().tobytes() and l1.cpu().numpy().tobytes() == l12.cpu().numpy().tobytes(), what
            worst = max(worst, sr.check_pairs(x.cpu().numpy(), l1.cpu().numpy(), c, what))
            if guard == GUARD:
                vx, vl1 = ops.stitch_pairs(view, ra, rb, c["margin"])
                assert vx.cpu().numpy().tobytes() == x.cpu().numpy().tobytes() and vl1.cpu().numpy().tobytes() == l1.cpu().numpy().tobytes(), what
    print(f"{c['name']}: l1 worst error / bound {worst:.3g} (chain {sr.chain(c['r'] - 3 * c['margin'])})")


@pytest.mark.parametrize("c", CROPS, ids=[c["name"] for c in CROPS])
def test_crops_kernel_against_the_statement(eng, c):
    ops = eng["ops"]
    dr, ix, off = (torch.from_numpy(c[k]).to("cuda") for k in ("drawings", "draw", "off"))
    n, r, (k, d) = len(c["draw"]), c["r"], c["drawings"].shape[:2]
    want = sr.crop_statement(c)
    got = []
    for guard in (GUARD, GUARD - 1, GUARD):
        out = Guarded(n * r * r, torch.float32, 777.0, guard)
        _lib.check(_lib.lib().nb_stitch_crops_u8(dr.data_ptr(), k, d, ix.data_ptr(), off.data_ptr(), n, r, out.view.data_ptr(), _stream()), "stitch_crops")
        torch.cuda.synchronize()
        assert out.intact()
        got.append(out.view.view(n, 1, r, r).cpu().numpy())
        assert got[-1].tobytes() == want.tobytes(), (c["name"], guard)
    assert ops.stitch_crops(dr, ix, off, r).cpu().numpy().tobytes() == want.tobytes()
    # indices and windows outside their range are clamped on the device
    far = ops.stitch_crops(dr, ix + 100, off - 1000, r).cpu().numpy()
    assert np.array_equal(far[:, 0], sr.u8_over_255()[c["drawings"][k - 1, :r, :r]][None].repeat(n, 0))
    assert tuple(ops.stitch_crops(dr, ix[:0], off[:0], r).shape) == (0, 1, r, r)


def test_empty_batch_and_bad_rectangles(eng):
    """n = 0 gives empty outputs; rectangles far outside the image composite nothing and read nothing outside the images."""
    ops = eng["ops"]
    c = next(x for x in CASES if x["name"] == "r32_m2_n5")
    fake, ra, rb = sr.to_torch(c, "cuda")
    x, l1 = ops.stitch_pairs(fake[:0], ra[:0], rb[:0], 2)
    assert tuple(x.shape) == (0, 3, 26, 26) and tuple(l1.shape) == (0,)
    wild = ra.clone()
    wild[0] = torch.tensor([-5, 0, 1 << 30, 9, 0, 0, 4, 4], dtype=torch.int32)
    wild[1] = torch.tensor([0, 0, 8, 8, -(1 << 30), 1 << 30, 8 - (1 << 30), 8 + (1 << 30)], dtype=torch.int32)
    none = ra.clone()
    none[:2] = 0
    a, b = ops.stitch_pairs(fake, wild, rb, 2), ops.stitch_pairs(fake, none, rb, 2)
    torch.cuda.synchronize()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---------------------------------------------------------------------------------------------------------------------
# pair_distance on the kernel's pairs
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch,s", sorted(sr.DISTANCE_CASES))
def test_pair_distance_on_kernel_made_pairs(eng, arch, s):
    """Slim ``alex`` and ``vgg`` at S = 52 (R = 64, margin 4) and S = 226 (R = 256, margin 10) on the pairs the kernel makes, against
    ``lpips_f64`` of the same float32 pairs, with the tolerance of tests/test_hip_metric_patches.py: SPLIT_F16_FACTOR x the float32
    torch route's error plus the ulp floor (the kink margins of that file's small case cannot hold at these sizes; stitch_refs has the
    reason)."""
    ops = eng["ops"]
    c = sr.distance_case(arch, s)
    sl = lr.SLIM[arch]
    w = lr.slim_weights(arch, sl["channels"], sl["seed"], sl["size"])
    x, l1 = ops.stitch_pairs(*sr.to_torch(c, "cuda"), c["margin"])
    xh = x.cpu().numpy()
    sr.check_pairs(xh, l1.cpu().numpy(), c)
    assert xh.shape == (4, 3, s, s) and not np.array_equal(xh[0], xh[2]) and not np.array_equal(xh[1], xh[3])
    want = mp.distance_f64(w, xh)
    t32 = lr.lpips_f64(w, xh[:2], xh[2:], dtype=torch.float32).numpy()
    tol = lr.SPLIT_F16_FACTOR * float(np.abs(t32.astype(np.float64) - want).max()) + cr.ULP_FLOOR * cr.EPS32 * np.abs(want)
    net = eng["net"] if arch == "alex" else perceptual.LPIPS(w, route="hip")
    got = net.pair_distance(x)
    torch.cuda.synchronize()
    e = np.abs(got.cpu().numpy().astype(np.float64) - want)
    print(f"[pair_distance] {arch} {s}: {got.cpu().numpy()}, error {e.max():.3g}, float32 torch route {np.abs(t32 - want).max():.3g}, bound {tol.min():.3g}")
    assert got.shape == (2,) and np.all(e <= tol), (arch, s, got, want)
    assert torch.equal(net.pair_distance(x), got)


# ---------------------------------------------------------------------------------------------------------------------
# the evaluator on the HIP engine
# ---------------------------------------------------------------------------------------------------------------------
def _noisy_library(eng):
    """Two z brushes and a W+ brush that carries noise buffers."""
    lib, cfg = eng["lib"], eng["cfg"]
    ids = lib.get_style_ids()
    from brush_noise_refs import fixture_buffers
    bufs = {k: torch.from_numpy(v) for k, v in fixture_buffers(load_golden("engine_brush_noise_r128.npz"), cfg).items()}

    class NoisyLibrary:
        def get_style_ids(self):
            return [ids[0], ids[1], "noisy"]

        def set_style(self, sid, opts):
            if sid != "noisy":
                return lib.set_style(sid, opts)
            opts.set_style_w(torch.from_numpy(eng["g"]["w_brush_ws"]), "noisy", custom_args={"noise_buffers": bufs})
    return NoisyLibrary()


def test_evaluator_with_stitch(eng):
    """Three brushes, one of them W+ with noise buffers, two rounds: STITCH_* held to the float64 statement on the images the passes
    rendered; the first pass's images equal a direct ``render_img`` of the plan's crops and positions as bytes; positions2 - positions1
    is the crop delta; the seven other columns are those of a run without ``stitch``, bit for bit."""
    evaluator, ops, net, w = eng["evaluator"], eng["ops"], eng["net"], eng["w"]
    library = _noisy_library(eng)
    setup = metrics.StitchSetup(eng["full"], MARGIN, MIN_OVERLAP)
    seen, ordinary = [], []

    def hook(units, renders, targets, stitch=None, own_renders=None):
        if stitch is None:
            ordinary.append(list(units))
        else:
            assert renders is None and targets is None
            seen.append(dict(stitch, fake=stitch["fake"].cpu().numpy()))
    with torch.no_grad():
        got = evaluator.evaluate(library, rounds=2, batch=4 * KS, lpips=net, stitch=setup, on_pass=hook)
        again = evaluator.evaluate(library, rounds=2, batch=4 * KS, lpips=net, stitch=setup)
        plain = evaluator.evaluate(library, rounds=2, batch=4 * KS, lpips=net)
    assert [p["units"] for p in seen] == [[(0, 0), (0, 1)], [(1, 0), (1, 1)], [(2, 0), (2, 1)]]
    assert ordinary == [[(0, 0), (0, 1)], [(1, 0), (1, 1)], [(2, 0), (2, 1)]]
    assert got.keys() == metrics.KEYS + metrics.PERCEPTUAL_KEYS + metrics.STITCH_KEYS and plain.stitching is None
    for key in got.keys():
        assert got.as_dict()[key].tobytes() == again.as_dict()[key].tobytes(), key
    for key in metrics.KEYS + metrics.PERCEPTUAL_KEYS:
        assert got.as_dict()[key].tobytes() == plain.as_dict()[key].tobytes(), key
    plan = metrics.default_stitch_plan(br.EVAL_SEED, 3, 2, KS, 128, D_FULL, MARGIN, MIN_OVERLAP)
    s = 128 - 3 * MARGIN
    dist64 = lambda x: lr.lpips_f64(w, x[:len(x) // 2], x[len(x) // 2:]).numpy()
    dist32 = lambda x: lr.lpips_f64(w, x[:len(x) // 2], x[len(x) // 2:], dtype=torch.float32).numpy()
    want, t32 = np.zeros((3, 2, 2)), np.zeros((3, 2, 2))
    for p in seen:
        b = p["units"][0][0]
        assert np.array_equal(p["crop1"], plan["crop1"][b]) and np.array_equal(p["crop2"], plan["crop2"][b])
        assert np.array_equal(p["positions1"], plan["positions1"][b].reshape(2 * KS, 2))
        assert np.array_equal(p["positions2"] - p["positions1"], np.repeat(p["crop2"] - p["crop1"], KS, 0))
        assert p["fake"].shape == (4 * KS, 3, 128, 128) and np.all(np.isfinite(p["fake"]))
        rects = [sr.crop_pair_rects((*p["crop1"][u], 128, 128), (*p["crop2"][u], 128, 128), MARGIN) for u in range(2)]
        ra, rb = (np.repeat(np.stack([q[j] for q in rects]), KS, 0) for j in range(2))
        want[b, :, 0], want[b, :, 1] = sr.scores_from_fake(p["fake"], ra, rb, MARGIN, KS, dist64)
        t32[b, :, 0], t32[b, :, 1] = sr.scores_from_fake(p["fake"], ra, rb, MARGIN, KS, dist32)
    want, t32 = want.mean(axis=1), t32.mean(axis=1)
    l1, lp = got.stitching["STITCH_L1"].astype(np.float64), got.stitching["STITCH_LPIPS"].astype(np.float64)
    tol_l1 = sr.l1_bound(want[:, 0], s) + 4 * sr.EPS32 * want[:, 0]         # (the sums' bound, averaged; four roundings to the score)
    e32 = float(np.abs(t32[:, 1] - want[:, 1]).max())
    tol_lp = lr.SPLIT_F16_FACTOR * e32 + cr.ULP_FLOOR * cr.EPS32 * np.abs(want[:, 1])
    print(f"[evaluator] STITCH_L1 {l1}, error {np.abs(l1 - want[:, 0]).max():.3g}, bound {tol_l1.min():.3g}")
    print(f"[evaluator] STITCH_LPIPS {lp}, error {np.abs(lp - want[:, 1]).max():.3g}, float32 torch route {e32:.3g}, bound {tol_lp.min():.3g}")
    assert np.all(want > 0) and np.all(np.abs(l1 - want[:, 0]) <= tol_l1) and np.all(np.abs(lp - want[:, 1]) <= tol_lp)
    assert np.abs(seen[2]["fake"]).max() > 0 and not np.array_equal(seen[0]["fake"], seen[1]["fake"])
    # the first pass again, by hand: the plan's windows, encoded, both sides in one positioned pass
    p = seen[0]
    from brushstroke_engine_amd.painting import GanBrushOptions
    opts = GanBrushOptions()
    library.set_style(library.get_style_ids()[0], opts)
    with torch.no_grad():
        wsb = ops.map_style(z=opts.style_z, ws=opts.style_ws).repeat_interleave(2 * KS, 0).repeat(2, 1, 1).contiguous()
        draw = torch.arange(KS, dtype=torch.int32, device="cuda").repeat(4)
        offs = torch.from_numpy(np.concatenate([np.repeat(p["crop1"], KS, 0), np.repeat(p["crop2"], KS, 0)]).astype(np.int32)).to("cuda")
        geo = ops.stitch_crops(torch.from_numpy(eng["full"]).to("cuda"), draw, offs)
        assert geo.cpu().numpy().tobytes() == np.stack([sr.u8_over_255()[eng["full"][d, y:y + 128, x:x + 128]] for d, (y, x) in
                                                        zip(draw.tolist(), offs.tolist())])[:, None].tobytes()
        pos = torch.from_numpy(np.concatenate([p["positions1"], p["positions2"]]).astype(np.int64)).to("cuda")
        direct = ops.render_img(wsb, ops.encode(geo), pos)
        torch.cuda.synchronize()
    assert direct.cpu().numpy().tobytes() == p["fake"].tobytes()


def test_main_writes_nine_columns_with_stitch_drawings(eng, tmp_path):
    """``brush_metrics_main --lpips_weights --stitch_drawings``: the two text files with the nine sorted columns in the reference's
    format, and the numbers of the evaluator with the same network, seed and default plans."""
    snap, drawings, wpath, full = (str(tmp_path / f) for f in ("engine.npz", "drawings.npz", "alex_slim.npz", "full.npz"))
    formats.save_engine_snapshot(snap, eng["cfg"], eng["sd"], eng["esd"], preproc_type=None)
    np.savez(drawings, drawings=eng["e"]["uvs_cal_medium"])
    np.savez(wpath, **eng["w"])
    np.savez(full, drawings=eng["full"])
    style, summary, info = brush_metrics_main.main(["--gan_checkpoint", snap, "--library", "594,0", "--drawings", drawings, "--output_dir",
                                                    str(tmp_path / "scores"), "--conv_mode", "h3", "--batch", "12", "--lpips_weights", wpath,
                                                    "--stitch_drawings", full, "--stitch_margin", str(MARGIN), "--stitch_min_overlap", str(MIN_OVERLAP)])
    keys = list(metrics.KEYS + metrics.PERCEPTUAL_KEYS + metrics.STITCH_KEYS)
    rows = open(style).read().splitlines(keepends=True)
    assert rows[0] == "SEED            " + metrics.file_line(keys) and [r.split()[0] for r in rows[1:]] == ["0", "594"]
    assert all(len(r) == len(rows[0]) and len(r.split()) == 10 for r in rows)
    top = open(summary).read().splitlines(keepends=True)
    assert top[0] == metrics.file_line(keys) and len(top) == 2 and len(top[1].split()) == 9 and len(top[1]) == len(top[0])
    back = json.load(open(info))
    assert back["ids"] == ["0", "594"] and list(back["metrics"]) == keys
    with torch.no_grad():
        s = eng["evaluator"].evaluate(eng["lib"], style_ids=["0", "594"], batch=12, lpips=eng["net"],
                                      stitch=metrics.StitchSetup(eng["full"], MARGIN, MIN_OVERLAP))
    for key in keys:
        assert np.array_equal(np.array(back["metrics"][key], np.float32), s.as_dict()[key]), key
