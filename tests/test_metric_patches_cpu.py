"""The inputs of the perceptual brush scores without a GPU: the float32 torch restatements of ``TileOpsBase`` against the float64
statement of tests/metric_patches_refs.py, the statement against its wrong variants, the plan, ``LPIPS.pair_distance`` on the torch
route, the evaluator on the oracle-backed ops, the files with and without the perceptual columns, and the entries' host checks."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import brush_catalogue_cases as bc
import brush_metrics_refs as br
import clarity_refs as cr
import lpips_refs as lr
import metric_patches_refs as mp
from conftest import load_golden
from brushstroke_engine_amd import _lib, brush_metrics_main, build, config as cfgmod, encoder as encmod, metrics, perceptual, tile_ops, weights as wmod
from oracle_tile_ops import OracleTileOps

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = mp.pair_cases()
IDS = [c["name"] for c in CASES]
OPS = tile_ops.TileOpsBase()


def _restated(c):
    ren, geom, o0, o1, s1 = mp.to_torch(c)
    g = OPS.bg_guidance(geom)
    mean = OPS.bg_mean_colors(ren, g)
    x = OPS.metric_pairs(ren, g if c["masked"] else None, mean if c["masked"] else None, o0, o1, s1, c["p"], c["transpose"], c["masked"])
    return g, mean, x


# ---------------------------------------------------------------------------------------------------------------------
# the statement and its cases
# ---------------------------------------------------------------------------------------------------------------------
def test_no_drawing_of_the_cases_leaves_a_pixel_undecided():
    """One blur at 0.99: every drawing set of brush_metrics_refs.cases() (R = 8, 20, 33, 128) and of the distance cases has zero
    undecided pixels; the smallest gap is 1.8e-5, at R = 33."""
    gaps = {}
    for name, g in list(br.mask_drawings().items()) + [(f"distance_{a}", mp.distance_case(a)[0]["geom_u8"]) for a in mp.DISTANCE_CASES]:
        blur1, _, _, und = mp.guidance_f64(br.geom_f32(g))
        assert not und.any(), name
        gaps[name] = float(np.abs(blur1 - mp.BG_THRESH).min())
    assert min(gaps.values()) > mp.UNDECIDED and min(gaps, key=gaps.get).startswith("r33") and 1.7e-5 < min(gaps.values()) < 1.9e-5, gaps
    cal = float(np.abs(mp.guidance_f64(br.geom_f32(br.cal_drawings()))[0] - mp.BG_THRESH).min())
    assert cal > 3e-3, cal                                                  # uvs_cal_medium, the evaluator's drawings: 4e-3


def test_cases_tell_the_wrong_variants_apart():
    """Each wrong variant differs from the statement by far more than the tolerance on at least one case, and the cases cover what
    the issue lists: odd p, both extreme offsets, a permutation onto another drawing, no background, only background, p = r."""
    worst = {w: 0.0 for w in mp.WRONG}
    for c in CASES:
        ref = mp.statement(c)
        for w in mp.WRONG:
            worst[w] = max(worst[w], float(np.abs(mp.statement(c, w)["x"] - ref["x"]).max()))
    assert all(v > 1000 * mp.FILL_TOL for v in worst.values()), worst
    by = {c["name"]: c for c in CASES}
    c = by["r33_n7_k5_p26"]
    assert any(int(j) % 5 != i % 5 for i, j in enumerate(c["src1"])) and c["p"] % 2 == 0 and (c["p"] * c["p"]) % 4 == 0
    assert by["r20_n7_k5_p7"]["p"] % 2 == 1 and (7 * 7) % 4 != 0
    for name in ("r20_n7_k5_p16", "r20_n7_k5_p7", "r33_n7_k5_p26"):
        c = by[name]
        lim = c["geom_u8"].shape[-1] - c["p"]
        both = np.concatenate([c["off0"], c["off1"]])
        assert 0 in both and lim in both and len({tuple(o) for o in c["off0"]}) > 1, name
    assert mp.statement(by["r20_n5_k1_all_stroke"])["filled"].all() and not mp.statement(by["r20_n5_k1_all_stroke"])["n_bg"].any()
    assert not mp.statement(by["r20_n1_k1_all_background"])["filled"].all()
    assert by["r33_n7_k5_p33_across"]["p"] == 33 and not by["r33_n7_k5_p33_across"]["masked"]


def test_tolerances_are_the_derived_ones():
    assert mp.BLUR1_TOL == 2e-6 and 26 * mp.U < mp.BLUR1_TOL < br.BLUR_TOL
    assert mp.PIXEL_TOL == 2.0 ** -21 and mp.MEAN_TOL == 68 * 2.0 ** -24 and mp.FILL_TOL == 2 * mp.MEAN_TOL + 2.0 ** -24


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_restatements_against_float64(c):
    ref = mp.statement(c)
    g, mean, x = _restated(c)
    mp.check_guidance(g.blur1.numpy(), g.n_bg.numpy(), br.geom_f32(c["geom_u8"]), c["name"])
    mp.check_mean(mean.numpy(), ref, c["name"])
    mp.check_pairs(x.numpy(), ref, c["name"])
    n = c["renders"].shape[0]
    assert x.shape == (2 * n, 3, c["p"], c["p"]) and x.dtype == torch.float32 and x.is_contiguous()
    if not c["masked"] and not c["transpose"]:                              # compute_lpips_across_geo's form: on white * 2 - 1 and its permutation
        proc = tile_ops.on_white_f32(torch.from_numpy(c["renders"])) * 2 - 1.0
        assert torch.equal(x[:n], proc) and torch.equal(x[n:], proc[torch.from_numpy(c["src1"]).long()])


def test_restatement_shape_checks():
    c = CASES[1]
    ren, geom, o0, o1, s1 = mp.to_torch(c)
    g = OPS.bg_guidance(geom)
    mean = OPS.bg_mean_colors(ren, g)
    for bad in (lambda: OPS.bg_guidance(geom.double()), lambda: OPS.bg_guidance(geom[:, :, :4]), lambda: OPS.bg_mean_colors(ren[:, :3], g),
                lambda: OPS.bg_mean_colors(ren[:, :, :8, :8], g), lambda: OPS.metric_pairs(ren, g, mean, o0, o1, s1, 0),
                lambda: OPS.metric_pairs(ren, g, mean, o0, o1, s1, 21), lambda: OPS.metric_pairs(ren, g, mean, o0.long(), o1, s1, 7),
                lambda: OPS.metric_pairs(ren, g, mean, o0[:3], o1, s1, 7), lambda: OPS.metric_pairs(ren, g, mean[:2], o0, o1, s1, 7),
                lambda: OPS.metric_pairs(ren, None, None, o0, o1, s1, 7), lambda: OPS.metric_pairs(ren, g, mean, o0, o1, o0[:, 0].float(), 7)):
        with pytest.raises(ValueError):
            bad()
    assert OPS.metric_pairs(ren, None, None, o0, o1, None, 7, True, False).shape == (14, 3, 7, 7)


# ---------------------------------------------------------------------------------------------------------------------
# the window width and the plan
# ---------------------------------------------------------------------------------------------------------------------
def test_default_patch_width():
    """geom_metric.py:224-229."""
    assert [metrics.default_patch_width(r) for r in (256, 128, 64, 32, 8)] == [64, 64, 51, 25, 6]
    assert metrics.default_patch_width(33) == 26 and metrics.default_patch_width(512) == 128 and metrics.default_patch_width(255) == 127


def test_default_crops():
    a, b = metrics.default_crops(5, 3, 2, 5, 128, 64), metrics.default_crops(5, 3, 2, 5, 128, 64)
    assert sorted(a) == sorted(metrics.CROP_KEYS)
    assert all(np.array_equal(a[k], b[k]) and a[k].dtype == np.int32 for k in a)
    other = metrics.default_crops(6, 3, 2, 5, 128, 64)
    assert any(not np.array_equal(a[k], other[k]) for k in a)
    for k in ("multi_off0", "multi_off1", "same_off0", "same_off1"):       # ONE offset pair per unit, inside the image
        assert a[k].shape == (3, 2, 2) and a[k].min() >= 0 and a[k].max() <= 64
    for k in ("same_perm", "geo_perm"):
        assert a[k].shape == (3, 2, 5) and np.array_equal(np.sort(a[k], axis=-1), np.broadcast_to(np.arange(5), (3, 2, 5)))
    # the documented order of draws from a CPU generator seeded seed + 2
    gen = torch.Generator().manual_seed(7)
    for name in ("multi_off0", "multi_off1", "same_off0", "same_off1"):
        assert np.array_equal(a[name][0, 0], torch.randint(0, 65, (2,), generator=gen).numpy())
    for name in ("same_perm", "geo_perm"):
        assert np.array_equal(a[name][0, 0], torch.randperm(5, generator=gen).numpy())
    assert np.array_equal(a["multi_off0"][0, 1], torch.randint(0, 65, (2,), generator=gen).numpy())
    full = metrics.default_crops(0, 2, 1, 5, 33, 33)                        # p = r: only offset 0
    assert not full["multi_off0"].any() and not full["same_off1"].any()
    with pytest.raises(ValueError):
        metrics.default_crops(0, 1, 1, 5, 32, 33)
    # over many units every offset of the range appears: randint's high end is exclusive at r - p + 1
    many = metrics.default_crops(1, 200, 1, 2, 20, 16)["multi_off0"]
    assert set(np.unique(many)) == set(range(5))


# ---------------------------------------------------------------------------------------------------------------------
# pair_distance
# ---------------------------------------------------------------------------------------------------------------------
def test_trunk_minimum_sizes():
    assert perceptual.min_size("alex") == 31 and perceptual.min_size("vgg") == 16
    for arch, need in (("alex", 31), ("vgg", 16)):
        s = lr.SLIM[arch]
        w = lr.slim_weights(arch, s["channels"], s["seed"], s["size"])
        net = perceptual.LPIPS(w, route="torch", device="cpu")
        with pytest.raises(ValueError, match="minimum side"):
            net.pair_distance(torch.zeros([2, 3, need - 1, need - 1]))
        assert net.pair_distance(torch.rand([2, 3, need, need]) * 2 - 1).shape == (1,)
        with pytest.raises(Exception):                                     # ... and one below the minimum the trunk itself has no window
            net(torch.zeros([1, 3, need - 1, need - 1]), torch.zeros([1, 3, need - 1, need - 1]))
        with pytest.raises(ValueError):
            net.pair_distance(torch.zeros([3, 3, 64, 64]))
        assert net.pair_distance(torch.zeros([0, 3, 64, 64])).shape == (0,)


@pytest.mark.parametrize("arch", sorted(mp.DISTANCE_CASES))
def test_pair_distance_torch_route(arch):
    """On the restated pairs of the distance case, against ``lpips_f64`` of the same float32 pairs, within ``bound``; the margins
    the GPU test relies on hold; one trunk pass; equal to the two-image call."""
    c, w = mp.distance_case(arch)
    assert c["p"] == metrics.default_patch_width(c["geom_u8"].shape[-1]) == lr.SLIM[arch]["size"]
    _, _, x = _restated(c)
    min_pre, min_gap, err = mp.pair_margins(w, x.numpy())
    print(f"{arch}: |pre| {min_pre / err:.0f} errors, pool gap {min_gap / err:.0f} errors")
    assert min_pre >= lr.KINK_MARGIN * err and min_gap >= lr.KINK_MARGIN * err
    want = mp.distance_f64(w, x.numpy())
    n = x.shape[0] // 2
    t32 = lr.lpips_f64(w, x[:n], x[n:], dtype=torch.float32).numpy()
    net = perceptual.LPIPS(w, route="torch", device="cpu")
    calls = net.trunk_calls
    got = net.pair_distance(x)
    assert net.trunk_calls == calls + 1 and got.shape == (n,) and got.dtype == torch.float32 and not got.requires_grad
    assert np.all(np.abs(got.numpy().astype(np.float64) - want) <= cr.bound(t32, want)), (got, want)
    two = net(x[:n], x[n:])
    assert np.all(np.abs(two.numpy().astype(np.float64) - want) <= cr.bound(t32, want))
    assert np.all(want > 1e-3)                                              # (the pairs do differ)


def test_reference_functions_on_the_restatement():
    """``compute_uniform_bg_lpips_metric`` and ``compute_lpips_across_geo`` with the reference's keys and return shapes."""
    c, w = mp.distance_case("alex")
    net = perceptual.LPIPS(w, route="torch", device="cpu")
    ren, geom, o0, o1, s1 = mp.to_torch(c)
    k, n = geom.shape[0], ren.shape[0]
    g_n = geom[torch.arange(n) % k].unsqueeze(1)
    crops = (tuple(c["off0"][0]), tuple(c["off1"][0]), c["src1"].tolist())
    res, dbg = metrics.compute_uniform_bg_lpips_metric(ren, g_n, net, same_style=True, crops=crops)
    shared = dict(c, geom_u8=c["geom_u8"][np.arange(n) % k], off0=np.repeat(c["off0"][:1], n, 0), off1=np.repeat(c["off1"][:1], n, 0))
    want = mp.distance_f64(w, mp.statement(shared)["x"]).mean()
    assert dbg is None and list(res) == ["LPIPS_UNIFORM_BG"] and abs(res["LPIPS_UNIFORM_BG"] - want) <= 1e-5 * want
    res, _ = metrics.compute_uniform_bg_lpips_metric(ren, g_n, net, patch_width=40, key_suffix="multicolor")
    assert list(res) == ["LPIPS_UNIFORM_BG_multicolor"] and res["LPIPS_UNIFORM_BG_multicolor"] > 0
    res = metrics.compute_lpips_across_geo(ren, net, perm=c["src1"].tolist())
    zero = np.zeros((n, 2), np.int32)
    want = mp.distance_f64(w, mp.statement(dict(c, p=128, transpose=False, masked=False, off0=zero, off1=zero))["x"]).mean()
    assert list(res) == ["LPIPS_ACROSS_GEO"] and abs(res["LPIPS_ACROSS_GEO"] - want) <= 1e-5 * want
    torch.manual_seed(0)
    assert metrics.compute_lpips_across_geo(ren, net)["LPIPS_ACROSS_GEO"] >= 0


# ---------------------------------------------------------------------------------------------------------------------
# the evaluator on the oracle-backed ops
# ---------------------------------------------------------------------------------------------------------------------
def test_evaluator_with_lpips_on_the_oracle_ops():
    e, g = load_golden("engine_r128.npz"), load_golden("brush_catalogue_r128.npz")
    cfg = cfgmod.style1_config(int(g["resolution"]))
    ops = OracleTileOps(cfg, wmod.random_state_dict(cfg, seed=int(g["weights_seed"])), encmod.random_encoder_state_dict(int(g["encoder_seed"])))
    lib = bc.FixtureLibrary(g, cfg.z_dim)
    ids = lib.get_style_ids()[:2]
    s = lr.SLIM["alex"]
    w = lr.slim_weights("alex", s["channels"], s["seed"], s["size"])
    net = perceptual.LPIPS(w, route="torch", device="cpu")
    evaluator = metrics.BrushEvaluator(ops, e["uvs_cal_medium"], seed=br.EVAL_SEED)
    seen, old = [], []
    got = evaluator.evaluate(lib, style_ids=ids, batch=10, lpips=net,
                             on_pass=lambda u, r, t, own_renders=None: seen.append((list(u), r.numpy().copy(), own_renders.numpy().copy())))
    plain = evaluator.evaluate(lib, style_ids=ids, batch=10, on_pass=lambda u, r, t: old.append(list(u)))
    kept = evaluator.evaluate(lib, style_ids=ids, batch=10, lpips=net, on_pass=lambda u, r, t: old.append(list(u)))     # an old callback still works
    assert [u for u, _, _ in seen] == [[(0, 0), (1, 0)]] and old == [[(0, 0), (1, 0)]] * 2
    assert plain.perceptual is None and plain.keys() == metrics.KEYS and got.keys() == metrics.KEYS + metrics.PERCEPTUAL_KEYS
    for key in metrics.KEYS:                                                # the four existing scores: bit for bit
        assert got.as_dict()[key].tobytes() == plain.as_dict()[key].tobytes(), key
    assert list(got.as_dict()) == sorted(got.as_dict()) == list(got.keys())
    plan = metrics.default_crops(br.EVAL_SEED, 2, 1, 5, 128, 64)
    want = mp.scores_from_passes(w, e["uvs_cal_medium"], seen, 2, 1, plan, 64)
    t32 = mp.scores_from_passes(w, e["uvs_cal_medium"], seen, 2, 1, plan, 64, dist=lambda x: lr.lpips_f64(
        w, x[:len(x) // 2].astype(np.float32), x[len(x) // 2:].astype(np.float32), dtype=torch.float32).numpy())
    for key in metrics.PERCEPTUAL_KEYS:
        v = got.perceptual[key]
        assert v.shape == (2,) and v.dtype == np.float32 and np.all(v > 0)
        assert np.all(np.abs(v.astype(np.float64) - want[key]) <= cr.bound(t32[key], want[key]) + 1e-6 * want[key]), (key, v, want[key])
        assert kept.perceptual[key].tobytes() == v.tobytes()
    assert not np.array_equal(seen[0][1], seen[0][2])                       # the second render has the brush's own colours
    assert got.rank("LPIPS_ACROSS_GEO")[0] == ids[int(np.argmin(got.perceptual["LPIPS_ACROSS_GEO"]))]
    empty = evaluator.evaluate(lib, style_ids=[], lpips=net)
    assert empty.ids == [] and sorted(empty.perceptual) == sorted(metrics.PERCEPTUAL_KEYS)
    with pytest.raises(ValueError):
        evaluator.evaluate(lib, style_ids=ids, lpips=net, crops={"multi_off0": plan["multi_off0"]})


# ---------------------------------------------------------------------------------------------------------------------
# BrushScores, the files and the command line
# ---------------------------------------------------------------------------------------------------------------------
def _scores(gold, perceptual_values=None):
    sample = dict(zip(metrics.KEYS, gold["file_sample_values"].tolist()))
    fields = {f: np.array([sample[k], sample[k] / 2], np.float32) for f, k in (("lab_e_percent", "LAB_E%"), ("lab_l2", "LAB_L2"),
                                                                               ("bg_clarity_mean", "BG_CLARITY_MEAN"), ("fg_opacity_median", "FG_OPACITY_MEDIAN"))}
    return metrics.BrushScores(["594", "7"], perceptual=perceptual_values, **fields)


def test_files_and_json_with_and_without_perceptual(tmp_path):
    gold = load_golden("brush_metrics.npz")
    assert metrics.PERCEPTUAL_KEYS == ("LPIPS_ACROSS_GEO", "LPIPS_UNIFORM_BG", "LPIPS_UNIFORM_BG_multicolor")
    assert list(metrics.KEYS + metrics.PERCEPTUAL_KEYS) == sorted(metrics.KEYS + metrics.PERCEPTUAL_KEYS)
    assert list(metrics.KEYS) == [str(k) for k in gold["file_keys"]]
    plain = _scores(gold)
    style, summary, info = brush_metrics_main.write_scores(plain, str(tmp_path / "a"))
    rows = open(style).read().splitlines(keepends=True)
    assert rows[0] == str(gold["file_style_header"]) and rows[1] == str(gold["file_sample_style_line"]) and len(rows) == 3
    top = open(summary).read().splitlines(keepends=True)
    assert top[0] == str(gold["file_summary_header"]) and len(top) == 2 and len(top[1].split()) == 4
    back = json.load(open(info))
    assert list(back) == ["ids", "metrics", "summary"] and list(back["metrics"]) == list(metrics.KEYS) == list(back["summary"])
    assert list(plain.as_dict()) == list(metrics.KEYS) and plain.rank("LAB_L2") == ["7", "594"]

    vals = {"LPIPS_ACROSS_GEO": np.array([0.25, 0.5], np.float32), "LPIPS_UNIFORM_BG": np.array([0.125, np.nan], np.float32),
            "LPIPS_UNIFORM_BG_multicolor": np.array([1.5, 0.03125], np.float32)}
    full = _scores(gold, vals)
    style, summary, info = brush_metrics_main.write_scores(full, str(tmp_path / "b"), "p_")
    rows = open(style).read().splitlines(keepends=True)
    keys = list(metrics.KEYS + metrics.PERCEPTUAL_KEYS)
    assert rows[0].split() == ["SEED"] + keys and rows[0].startswith(str(gold["file_style_header"])[:-1] + " ")
    assert rows[1].startswith(str(gold["file_sample_style_line"])[:-1] + " ") and all(len(r) == len(rows[0]) for r in rows)
    assert rows[1].split()[5:] == ["0.2500", "0.1250", "1.5000"] and rows[2].split()[5:] == ["0.5000", "nan", "0.0312"]
    top = open(summary).read().splitlines(keepends=True)
    assert top[0].split() == keys and len(top[1]) == len(top[0]) and top[1].split()[4:] == ["0.3750", "nan", "0.7656"]
    # every cell right-aligned under its key, in the reference's format (to_file_line: '{:>8}' cells joined by one blank)
    assert rows[0] == "SEED            " + metrics.file_line(keys)
    back = json.load(open(info))
    assert list(back["metrics"]) == keys == list(back["summary"]) and back["metrics"]["LPIPS_ACROSS_GEO"] == [0.25, 0.5]
    assert full.rank("LPIPS_UNIFORM_BG") == ["594", "7"] and full.rank("LPIPS_UNIFORM_BG_multicolor") == ["7", "594"]      # lower is better, NaN last


def test_parser_defaults():
    a = brush_metrics_main.build_parser().parse_args(["--gan_checkpoint", "e.npz", "--drawings", "d.npz", "--output_dir", "o"])
    assert (a.lpips_weights, a.lpips_net, a.patch_width) == (None, None, None)
    assert (a.library, a.rounds, a.batch, a.seed, a.lab_thresh, a.prefix, a.conv_mode, a.uvs_calibration) == ("rand100", 1, 32, 0, 10, "", None, None)
    b = brush_metrics_main.build_parser().parse_args(["--gan_checkpoint", "e.npz", "--drawings", "d.npz", "--output_dir", "o", "--lpips_weights", "w.npz",
                                                      "--lpips_net", "alex", "--patch_width", "48"])
    assert (b.lpips_weights, b.lpips_net, b.patch_width) == ("w.npz", "alex", 48)
    assert "alex" in brush_metrics_main.build_parser().format_help()
    with pytest.raises(SystemExit):
        brush_metrics_main.build_parser().parse_args(["--gan_checkpoint", "e.npz", "--drawings", "d.npz", "--output_dir", "o", "--lpips_net", "squeeze"])


# ---------------------------------------------------------------------------------------------------------------------
# the entries: host argument checks (before any HIP call, so no GPU is needed), header, prototypes, sources
# ---------------------------------------------------------------------------------------------------------------------
def test_entries_validate_on_the_host():
    build.build()
    lib = _lib.lib()
    f = (ctypes.c_float * 4096)()
    a = ctypes.addressof(f)
    i = ctypes.addressof((ctypes.c_int32 * 64)())

    def rejected(rc, text):
        assert rc == -1 and text.encode() in lib.nb_last_error(), (rc, lib.nb_last_error())

    rejected(lib.nb_bg_guidance_f32(None, 1, 8, a, i, None), "null pointer")
    rejected(lib.nb_bg_guidance_f32(a, -1, 8, a, i, None), "bad sizes")
    rejected(lib.nb_bg_guidance_f32(a, 1, 0, a, i, None), "bad sizes")
    rejected(lib.nb_bg_guidance_f32(a, 1, 8193, a, i, None), "bad sizes")
    rejected(lib.nb_bg_guidance_f32(a + 2, 1, 8, a, i, None), "4-byte aligned")
    assert lib.nb_bg_guidance_f32(a, 0, 8, a, i, None) == 0

    rejected(lib.nb_bg_mean_colors_f32(a, 256, a, i, 1, 8, 1, None, a, None), "null pointer")
    rejected(lib.nb_bg_mean_colors_f32(a, 256, a, i, 0, 8, 1, a, a, None), "bad sizes")
    rejected(lib.nb_bg_mean_colors_f32(a, 256, a, i, 1, 8, -1, a, a, None), "bad sizes")
    rejected(lib.nb_bg_mean_colors_f32(a, 255, a, i, 1, 8, 1, a, a, None), "alias")
    rejected(lib.nb_bg_mean_colors_f32(a, 256, a + 1, i, 1, 8, 1, a, a, None), "4-byte aligned")
    assert lib.nb_bg_mean_colors_f32(a, 256, a, i, 1, 8, 0, a, a, None) == 0

    pairs = lambda **kw: lib.nb_metric_pairs_f32(*[{**dict(renders=a, stride=256, blur1=a, mean=a, off0=i, off1=i, src1=None, k=1, r=8, p=6, n=1,
                                                           flags=3, out=a, stream=None), **kw}[key] for key in
                                                   ("renders", "stride", "blur1", "mean", "off0", "off1", "src1", "k", "r", "p", "n", "flags", "out", "stream")])
    rejected(pairs(renders=None), "null pointer")
    rejected(pairs(off1=None), "null pointer")
    rejected(pairs(out=None), "null pointer")
    rejected(pairs(blur1=None), "MASKED needs")
    rejected(pairs(mean=None, flags=2), "MASKED needs")
    rejected(pairs(flags=4), "unknown flags")
    rejected(pairs(p=0), "bad sizes")
    rejected(pairs(p=9), "bad sizes")
    rejected(pairs(k=0), "bad sizes")
    rejected(pairs(n=(1 << 24) + 1), "bad sizes")
    rejected(pairs(stride=255), "alias")
    rejected(pairs(out=a + 2), "4-byte aligned")
    rejected(pairs(r=8192, p=8192, stride=4 * 8192 * 8192, n=1 << 16), "exceed the grid")
    assert pairs(n=0) == 0 and pairs(n=0, blur1=None, mean=None, flags=1) == 0


def test_header_prototypes_and_sources():
    header = open(os.path.join(REPO, "include", "neube_hip.h")).read()
    for name in ("nb_bg_guidance_f32", "nb_bg_mean_colors_f32", "nb_metric_pairs_f32"):
        assert name in _lib.PROTOTYPES and re.search(r"\bint %s\(" % name, header), name
    assert len(_lib.PROTOTYPES["nb_metric_pairs_f32"][1]) == 14 and len(_lib.PROTOTYPES["nb_bg_mean_colors_f32"][1]) == 10
    assert re.search(r"#define NB_BG_MEAN_PARTS\s+%d\b" % _lib.NB_BG_MEAN_PARTS, header)
    assert re.search(r"#define NB_METRIC_PAIRS_TRANSPOSE\s+%d\b" % _lib.NB_METRIC_PAIRS_TRANSPOSE, header)
    assert re.search(r"#define NB_METRIC_PAIRS_MASKED\s+%d\b" % _lib.NB_METRIC_PAIRS_MASKED, header)
    for cite in ("geom_metric.py:207-262", "geom_metric.py:190-204", "geom_metric.py:238-239", "geom_metric.py:232-241", "geom_metric.py:250"):
        assert cite in header, cite
    assert "nb_metric_patches.hip" in build.SOURCES and build.FILE_FLAGS["nb_metric_patches.hip"] == ["-fno-slp-vectorize"]
    assert "# nb_metric_patches.hip: scalar fp32 per pixel" in open(os.path.join(REPO, "brushstroke_engine_amd", "build.py")).read()
    assert _lib.ABI_VERSION == 22
