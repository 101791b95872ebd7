"""The brush scores without a GPU: the float64 statement of tests/brush_metrics_refs.py against what the REFERENCE returned
(tests/golden/brush_metrics.npz), the torch routes of ``TileOpsBase`` and the functions of ``metrics`` against both, ``BrushEvaluator``
on the oracle-backed ops end to end, the C entries' argument checks and the files of ``brush_metrics_main``."""
import json
import os
import re

import numpy as np
import pytest
import torch

import brush_catalogue_cases as bc
import brush_metrics_refs as br
from brush_metrics_refs import _expand, _pooled_f64, check_against_passes, check_image_sums
from conftest import load_golden
from brushstroke_engine_amd import _lib, brush_metrics_main, config as cfgmod, encoder as encmod, metrics, painting, weights as wmod
from oracle_tile_ops import OracleTileOps

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = br.cases()
IDS = [c["name"] for c in CASES]


@pytest.fixture(scope="module")
def gold():
    return load_golden("brush_metrics.npz")


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_statement_matches_reference(gold, c):
    """The float64 statement against the reference's float32 results, within the reference's own error ``eps_ref``."""
    eps, name = float(gold["eps_ref"]), c["name"]
    g, _ = _expand(c)
    assert np.abs(gold[f"{name}/deltas"].astype(np.float64) - br.deltas_f64(c["targets"], c["renders"], c["ignore"])).max() <= eps
    blur, bg, fg, und = br.masks_f64(g)
    assert np.abs(gold[f"{name}/blur"].astype(np.float64) - blur).max() <= br.BLUR_TOL
    k, r = g.shape[0], g.shape[1]
    cbg = np.unpackbits(gold[f"{name}/conservative_bg"])[:k * r * r].reshape(k, 1, r, r)[:, 0].astype(bool)
    cfg_ = np.unpackbits(gold[f"{name}/conservative_fg"])[:k * r * r].reshape(k, 1, r, r)[:, 0].astype(bool)
    assert np.array_equal(cbg[~und], (blur >= br.BG_THRESH)[~und])
    near = np.abs(blur - 0.1) <= br.UNDECIDED
    assert np.array_equal(cfg_[~near], (blur < 0.1)[~near])
    s = gold[f"{name}/scalars"]
    got = {"BG_CLARITY_MEAN": s[0:1], "FG_OPACITY_MEDIAN": s[1:2].astype(np.float32), "LAB_E%": s[2:3], "LAB_L2": s[3:4]}
    br.check_scores(got, _pooled_f64(c, eps), eps / br.KERNEL_EPS_FACTOR, name)            # (the reference itself: 1 x eps_ref)


def test_eps_ref_is_the_stated_order(gold):
    """The issue measured 5.3e-5 on uniform random renders with dE up to 180; the committed cases give the same order."""
    assert 1e-5 < float(gold["eps_ref"]) < 5e-4


def test_drawings_leave_no_pixel_undecided():
    """No drawing of the cases has a float64 blur within 1e-5 of the background threshold: the mask comparison skips nothing.  And
    the border drawings tell the zero padding between the two applications from one 9x9 blur of a haloed tile."""
    seen = False
    for name, g8 in br.mask_drawings().items():
        g = br.geom_f32(g8)
        blur, bg, _, und = br.masks_f64(g)
        assert not und.any(), (name, int(und.sum()), float(np.abs(blur - br.BG_THRESH).min()))
        wrong = br.blur_9x9_wrong(g)
        if "border" in name:
            assert np.abs(wrong - blur).max() > 100 * br.BLUR_TOL, name
            seen = True
    assert seen
    g = br.geom_f32(np.full((1, 20, 20), 255, np.uint8))                                   # an empty drawing: the padding alone
    assert np.abs(br.blur_9x9_wrong(g) - br.masks_f64(g)[0]).max() > 1e-2


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_torch_routes(gold, c):
    """``TileOpsBase.eval_masks`` / ``brush_metrics`` (float32 torch, the reference's operations) against the float64 statement."""
    eps, name = float(gold["eps_ref"]), c["name"]
    ops = painting.TileOpsBase()
    g, _ = _expand(c)
    n, k, r = c["renders"].shape[0], g.shape[0], g.shape[1]
    m = ops.eval_masks(torch.from_numpy(g))
    br.check_masks(m.blur.numpy(), m.mask.numpy(), m.n_bg.numpy(), m.n_fg.numpy(), g, name)
    assert np.array_equal(m.blur.numpy(), gold[f"{name}/blur"])                            # the reference's own operations
    sums, alpha, deltas = ops.brush_metrics(torch.from_numpy(c["renders"]), torch.from_numpy(c["targets"]), m, c["lab_thresh"],
                                            c["ignore"], want_deltas=True)
    assert sums.shape == (n, 4) and alpha.shape == (n, r * r) and np.array_equal(alpha.numpy().reshape(n, r, r), c["renders"][:, 3])
    d64 = br.deltas_f64(c["targets"], c["renders"], c["ignore"])
    assert np.abs(deltas.numpy() - d64).max() <= br.KERNEL_EPS_FACTOR * eps
    assert np.array_equal(deltas.numpy(), gold[f"{name}/deltas"])
    check_image_sums(sums.numpy(), c, d64, eps)
    # a strided view and uint8 / bool-free inputs of the wrong kind
    big = torch.full([n, 6, r, r], float("nan"))
    big[:, 1:5] = torch.from_numpy(c["renders"])
    s2, a2 = ops.brush_metrics(big[:, 1:5], torch.from_numpy(c["targets"]), m, c["lab_thresh"], c["ignore"])
    assert torch.equal(s2, sums) and torch.equal(a2, alpha)
    with pytest.raises(ValueError):
        ops.brush_metrics(torch.from_numpy(c["renders"])[:, :3], torch.from_numpy(c["targets"]), m)
    with pytest.raises(ValueError):
        ops.brush_metrics(torch.from_numpy(c["renders"]), torch.from_numpy(c["targets"])[:, :2], m)


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_functions_match_reference(gold, c):
    """``metrics.compute_*`` keep the reference's signatures and keys and give its numbers."""
    eps, name = float(gold["eps_ref"]), c["name"]
    _, g_n = _expand(c)
    ren, tg, gt = torch.from_numpy(c["renders"]), torch.from_numpy(c["targets"]), torch.from_numpy(g_n)
    lab = metrics.compute_lab_metrics(tg, ren, gt, lab_thresh=c["lab_thresh"], ignore_transparency=c["ignore"])
    tr = metrics.compute_transparency_metrics(ren, gt)
    assert sorted(lab) == ["LAB_E%", "LAB_L2"] and sorted(tr) == ["BG_CLARITY_MEAN", "FG_OPACITY_MEDIAN"]
    assert all(isinstance(v, float) for v in list(lab.values()) + list(tr.values()))
    got = {k: np.array([v]) for k, v in {**lab, **tr}.items()}
    br.check_scores(got, _pooled_f64(c, br.KERNEL_EPS_FACTOR * eps), eps, name)
    s = gold[f"{name}/scalars"]
    np.testing.assert_allclose([tr["BG_CLARITY_MEAN"], lab["LAB_E%"], lab["LAB_L2"]], s[[0, 2, 3]], rtol=2e-6, atol=2e-6, equal_nan=True)
    assert np.array_equal(np.float32(tr["FG_OPACITY_MEDIAN"]), np.float32(s[1]), equal_nan=True)
    d = metrics.compute_lab_deltas(tg, ren, ignore_transparency=c["ignore"])
    assert np.array_equal(d.numpy(), gold[f"{name}/deltas"])


def test_lower_median():
    """``torch.median`` returns the LOWER median: of [3, 1, 2, 4] it is 2, and so is the k-th largest with k = N - (N - 1) // 2."""
    assert float(torch.median(torch.tensor([3.0, 1.0, 2.0, 4.0]))) == 2.0
    ren = torch.zeros([1, 4, 2, 2])
    ren[0, 3] = torch.tensor([[3.0, 1.0], [2.0, 4.0]]) / 4
    tr = metrics.compute_transparency_metrics(ren, torch.zeros([1, 1, 2, 2]))
    assert tr["FG_OPACITY_MEDIAN"] == 0.5 and np.isnan(tr["BG_CLARITY_MEAN"])


# ---------------------------------------------------------------------------------------------------------------------
# the evaluator on the oracle-backed ops
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ev():
    """The R=128 engine of tests/test_brush_catalogue_cpu.py, an evaluator on its five calibration drawings, and one evaluation of the
    four fixture brushes: two rounds, batch 10 (two units per pass), every pass's renders kept."""
    e, g = load_golden("engine_r128.npz"), load_golden("brush_catalogue_r128.npz")
    cfg = cfgmod.style1_config(int(g["resolution"]))
    ops = OracleTileOps(cfg, wmod.random_state_dict(cfg, seed=int(g["weights_seed"])), encmod.random_encoder_state_dict(int(g["encoder_seed"])))
    lib = bc.FixtureLibrary(g, cfg.z_dim)
    evaluator = metrics.BrushEvaluator(ops, e["uvs_cal_medium"], seed=br.EVAL_SEED)
    seen = []
    scores = evaluator.evaluate(lib, rounds=br.EVAL_ROUNDS, batch=10, on_pass=lambda u, r, t: seen.append((list(u), r.numpy().copy(), t.numpy().copy())))
    return dict(e=e, ops=ops, lib=lib, evaluator=evaluator, scores=scores, seen=seen)


def test_evaluator_scores_its_renders(gold, ev):
    s, seen = ev["scores"], ev["seen"]
    assert s.ids == ev["lib"].get_style_ids() and all(v.shape == (4,) and v.dtype == np.float32 for v in s.as_dict().values())
    assert [u for u, _, _ in seen] == [[(0, 0), (0, 1)], [(1, 0), (1, 1)], [(2, 0), (2, 1)], [(3, 0), (3, 1)]]
    assert all(r.shape == (10, 4, 128, 128) and t.shape == (10, 3) for _, r, t in seen)
    check_against_passes(s, seen, ev["e"]["uvs_cal_medium"], br.EVAL_ROUNDS, float(gold["eps_ref"]))
    assert np.all(np.isfinite(np.stack(list(s.as_dict().values()))))


def test_default_colors_are_the_reference_stream(gold, ev):
    stream = gold["color_stream"]                                           # 8 draws of (5, 3): brush-major, then rounds
    assert np.array_equal(metrics.default_colors(br.EVAL_SEED, 4, br.EVAL_ROUNDS, 5).reshape(8, 5, 3), stream)
    got = np.stack([t.reshape(-1, 5, 3) for _, _, t in ev["seen"]]).reshape(8, 5, 3)
    assert np.array_equal(got, stream)
    assert not np.array_equal(metrics.default_colors(br.EVAL_SEED + 1, 4, br.EVAL_ROUNDS, 5).reshape(8, 5, 3), stream)


def test_evaluator_batching_colours_and_functions(gold, ev):
    """One unit per pass gives the scores of two per pass; the functions give the evaluator's numbers on its renders; other target
    colours change LAB_L2 (the per-sample colours reach the render)."""
    eps, evaluator, lib = float(gold["eps_ref"]), ev["evaluator"], ev["lib"]
    ids = lib.get_style_ids()[:2]
    seen = []
    one = evaluator.evaluate(lib, style_ids=ids, rounds=1, batch=5, on_pass=lambda u, r, t: seen.append((list(u), r.numpy().copy(), t.numpy().copy())))
    assert [u for u, _, _ in seen] == [[(0, 0)], [(1, 0)]]
    cols = metrics.default_colors(br.EVAL_SEED, 2, 1, 5)
    two = evaluator.evaluate(lib, style_ids=ids, rounds=1, batch=32, colors=cols)
    for key in metrics.KEYS:                                                # (the oracle renders sample by sample: the same renders)
        assert np.array_equal(one.as_dict()[key], two.as_dict()[key], equal_nan=True), key
    check_against_passes(one, seen, ev["e"]["uvs_cal_medium"], 1, eps)
    geom = torch.from_numpy(br.geom_f32(ev["e"]["uvs_cal_medium"])).unsqueeze(1)
    for j, (_, ren, tg) in enumerate(seen):
        lab = metrics.compute_lab_metrics(torch.from_numpy(tg), torch.from_numpy(ren), geom, ops=ev["ops"])
        tr = metrics.compute_transparency_metrics(torch.from_numpy(ren), geom, ops=ev["ops"])
        got = one.as_dict()
        np.testing.assert_allclose([lab["LAB_E%"], lab["LAB_L2"], tr["BG_CLARITY_MEAN"]],
                                   [got["LAB_E%"][j], got["LAB_L2"][j], got["BG_CLARITY_MEAN"][j]], rtol=1e-6)
        assert np.float32(tr["FG_OPACITY_MEDIAN"]) == got["FG_OPACITY_MEDIAN"][j]
    other = evaluator.evaluate(lib, style_ids=ids, rounds=1, batch=32, colors=1 - cols)
    assert np.all(np.abs(other.lab_l2 - one.lab_l2) > 1e-3)
    with pytest.raises(ValueError):
        evaluator.evaluate(lib, style_ids=ids, colors=cols[:1])
    with pytest.raises(ValueError):
        metrics.BrushEvaluator(ev["ops"], ev["e"]["uvs_cal_medium"][:, :64, :64])
    assert evaluator.evaluate(lib, style_ids=[]).ids == []


def test_evaluator_with_uvs_mapper(ev):
    """With a mapper the brushes' factors come from one ``calibrate`` call and stretch the background weight: the background gets
    clearer (on this engine of random weights it is far from clear either way)."""
    e = ev["e"]
    mapper = painting.StyleUVSMapper(ev["ops"], e["uvs_cal_medium"], e["uvs_cal_thick"])
    calls = []
    calibrate = mapper.calibrate
    mapper.calibrate = lambda opts, batch=None: calls.append(len(opts)) or calibrate(opts, batch)
    mapped = metrics.BrushEvaluator(ev["ops"], e["uvs_cal_medium"], seed=br.EVAL_SEED, uvs_mapper=mapper)
    ids = ev["lib"].get_style_ids()[:2]
    cols = metrics.default_colors(br.EVAL_SEED, 4, br.EVAL_ROUNDS, 5)[:2, :1]
    s = mapped.evaluate(ev["lib"], style_ids=ids, rounds=1, batch=10, colors=cols)
    assert calls == [2] and sorted(mapper.sfactors) == sorted(ids)
    plain = ev["evaluator"].evaluate(ev["lib"], style_ids=ids, rounds=1, batch=10, colors=cols)
    assert np.all(s.bg_clarity_mean > plain.bg_clarity_mean)


# ---------------------------------------------------------------------------------------------------------------------
# BrushScores and the command line
# ---------------------------------------------------------------------------------------------------------------------
def test_scores_files_match_reference_format(gold, ev, tmp_path):
    assert list(metrics.KEYS) == [str(k) for k in gold["file_keys"]]
    sample = dict(zip(metrics.KEYS, gold["file_sample_values"].tolist()))
    one = metrics.BrushScores(["594"], **{f: np.array([sample[k]], np.float32) for f, k in
                                          (("lab_e_percent", "LAB_E%"), ("lab_l2", "LAB_L2"), ("bg_clarity_mean", "BG_CLARITY_MEAN"),
                                           ("fg_opacity_median", "FG_OPACITY_MEDIAN"))})
    style, summary = one.write_reference_files(str(tmp_path / "a"), "p_")
    assert os.path.basename(style) == "p_style_metrics.txt" and os.path.basename(summary) == "p_summary_metrics.txt"
    lines = open(style).read().splitlines(keepends=True)
    assert lines == [str(gold["file_style_header"]), str(gold["file_sample_style_line"])]
    lines = open(summary).read().splitlines(keepends=True)
    assert lines[0] == str(gold["file_summary_header"]) and lines[1] == str(gold["file_sample_style_line"])[16:]
    # the evaluated library through brush_metrics_main's writer
    s = ev["scores"]
    style, summary, info = brush_metrics_main.write_scores(s, str(tmp_path / "b"))
    rows = open(style).read().splitlines()
    assert rows[0] + "\n" == str(gold["file_style_header"]) and [r.split()[0] for r in rows[1:]] == [str(i) for i in s.ids]
    assert np.allclose([float(x) for x in rows[2].split()[1:]], [s.as_dict()[k][1] for k in metrics.KEYS], atol=5.1e-5)
    assert np.allclose([float(x) for x in open(summary).read().splitlines()[1].split()], [s.summary()[k] for k in metrics.KEYS], atol=5.1e-5)
    back = json.load(open(info))
    assert back["ids"] == [str(i) for i in s.ids] and sorted(back["metrics"]) == sorted(metrics.KEYS)
    assert np.array_equal(np.array(back["metrics"]["LAB_L2"], np.float32), s.lab_l2) and back["summary"] == s.summary()
    assert s.summary()["LAB_L2"] == pytest.approx(float(np.mean(s.lab_l2.astype(np.float64))))


def test_rank():
    s = metrics.BrushScores(["a", "b", "c"], lab_e_percent=np.array([5, 1, 3], np.float32), lab_l2=np.array([2, np.nan, 1], np.float32),
                            bg_clarity_mean=np.array([0.5, 0.9, np.nan], np.float32), fg_opacity_median=np.array([1, 0.2, 0.7], np.float32))
    assert s.rank("LAB_E%") == ["b", "c", "a"] and s.rank("LAB_L2") == ["c", "a", "b"]
    assert s.rank("BG_CLARITY_MEAN") == ["b", "a", "c"] and s.rank("FG_OPACITY_MEDIAN") == ["a", "c", "b"]
    assert np.isnan(s.summary()["LAB_L2"]) and s.summary()["LAB_E%"] == 3.0


def test_main_parser_and_drawings_file(tmp_path):
    args = brush_metrics_main.build_parser().parse_args(["--gan_checkpoint", "e.npz", "--drawings", "d.npz", "--output_dir", "o"])
    assert (args.library, args.rounds, args.batch, args.seed, args.lab_thresh, args.uvs_calibration, args.prefix) == ("rand100", 1, 32, 0, 10, None, "")
    d = np.random.RandomState(0).randint(0, 256, (2, 8, 8)).astype(np.uint8)
    np.savez(tmp_path / "d.npz", drawings=d)
    np.savez(tmp_path / "first.npz", d)
    assert np.array_equal(brush_metrics_main.load_drawings(str(tmp_path / "d.npz")), d)
    assert np.array_equal(brush_metrics_main.load_drawings(str(tmp_path / "first.npz")), d)


# ---------------------------------------------------------------------------------------------------------------------
# the C boundary
# ---------------------------------------------------------------------------------------------------------------------
def test_abi_22_and_header():
    common = open(os.path.join(REPO, "brushstroke_engine_amd", "csrc", "nb_common.h")).read()
    assert re.search(r"#define NB_ABI_VERSION (\d+)", common).group(1) == "22" and _lib.ABI_VERSION == 22
    assert _lib.lib().nb_abi_version() == 22
    header = open(os.path.join(REPO, "include", "neube_hip.h")).read()
    assert "nb_eval_masks_f32(" in header and "nb_brush_metrics_f32(" in header
    assert int(re.search(r"#define NB_BRUSH_METRICS_PARTS (\d+)", header).group(1)) == _lib.NB_BRUSH_METRICS_PARTS
    assert "nb_metrics.hip" in __import__("brushstroke_engine_amd.build", fromlist=["SOURCES"]).SOURCES


def test_c_entries_argument_checks():
    """Validation happens on the host before any HIP call: usable without a GPU."""
    library = _lib.lib()
    f = np.zeros(4 * 64 * 2 + 64, np.float32)
    b = np.zeros(64, np.uint8)
    i32 = np.zeros(4, np.int32)
    F, B, I = f.ctypes.data, b.ctypes.data, i32.ctypes.data

    def masks(geom=F, k=1, r=8, blur=F, mask=B, n_bg=I, n_fg=I):
        return library.nb_eval_masks_f32(geom, k, r, blur, mask, n_bg, n_fg, None)

    def bm(renders=F, stride=256, target=F, geom=F, mask=B, k=1, r=8, n=2, sums=F, alpha=F, deltas=None, partials=F):
        return library.nb_brush_metrics_f32(renders, stride, target, geom, mask, k, r, n, 10.0, 0, sums, alpha, deltas, partials, None)
    for call, bad, word in ((masks, dict(geom=None), "null"), (masks, dict(mask=None), "null"), (masks, dict(n_fg=None), "null"),
                            (masks, dict(k=-1), "k -1"), (masks, dict(r=0), "r 0"), (masks, dict(r=8193), "r 8193"),
                            (masks, dict(blur=F + 2), "aligned"),
                            (bm, dict(renders=None), "null"), (bm, dict(partials=None), "null"), (bm, dict(alpha=None), "null"),
                            (bm, dict(k=0), "k 0"), (bm, dict(r=0), "r 0"), (bm, dict(n=-1), "n -1"), (bm, dict(stride=255), "stride_n 255"),
                            (bm, dict(deltas=F + 1), "aligned"), (bm, dict(renders=F + 2), "aligned")):
        rc = call(**bad)
        assert rc == _lib.NB_EINVAL, bad
        assert word.encode() in library.nb_last_error(), (bad, library.nb_last_error())
    assert masks(k=0) == 0 and bm(n=0) == 0
