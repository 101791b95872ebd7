"""The stitching scores without a GPU: the torch restatements of ``TileOpsBase`` against the numpy statement of tests/stitch_refs.py, the
reference's recorded tensors (tests/golden/stitch_metrics.npz) and ``CropHelper.composite``; the plan; the files with nine columns; the
evaluator on the oracle-backed ops; what raises; and the entries' host checks."""
import ctypes
import fractions
import json
import os
import random
import re

import numpy as np
import pytest
import torch

import brush_catalogue_cases as bc
import brush_metrics_refs as br
import lpips_refs as lr
import stitch_refs as sr
from conftest import load_golden
from brushstroke_engine_amd import _lib, brush_metrics_main, build, config as cfgmod, encoder as encmod, metrics, perceptual, tile_ops, weights as wmod
from brushstroke_engine_amd.forger_losses import CropHelper, RandomStitcher
from oracle_tile_ops import OracleTileOps

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = sr.pair_cases()
IDS = [c["name"] for c in CASES]
CROPS = sr.crop_cases()
OPS = tile_ops.TileOpsBase()


# ---------------------------------------------------------------------------------------------------------------------
# the statement, the cases and the restatements
# ---------------------------------------------------------------------------------------------------------------------
def test_u8_over_255_is_correctly_rounded():
    """The table of the statement against the rational v / 255 rounded to the nearest float32 (ties cannot occur: checked)."""
    lut = sr.u8_over_255()
    for v in range(256):
        exact = fractions.Fraction(v, 255)
        got = fractions.Fraction(float(lut[v]))
        lo, hi = (fractions.Fraction(float(np.nextafter(lut[v], np.float32(s)))) for s in (-1, 2))
        assert abs(got - exact) < abs(lo - exact) and abs(got - exact) < abs(hi - exact), v


def test_cases_cover_what_the_issue_lists():
    names = set(IDS)
    kinds = set(sr.rect_kinds(32, 2))
    assert {"inside", "top", "bottom", "left", "right", "outside_top", "one_wide", "empty", "whole"} <= kinds
    assert all(f"r32_m2_n1_{q}" in names for q in kinds) and {"r32_m2_n5", "r32_m0_n5", "r33_m1_n5", "r256_m10_n1"} <= names
    by = {c["name"]: c for c in CASES}
    assert by["r256_m10_n1"]["r"] - 3 * by["r256_m10_n1"]["margin"] == 226 and by["r32_m2_n5"]["r"] - 6 == 26
    assert len({tuple(q) for q in by["r32_m2_n5"]["rects_a"].tolist()}) == 5          # they differ from sample to sample
    # a rectangle wholly outside the crop window: pairs equal, sum 0; one inside: pairs differ
    x, l1 = sr.statement(by["r32_m2_n1_outside_top"])
    assert np.array_equal(x[0], x[2]) and l1[0] == 0
    x, l1 = sr.statement(by["r32_m2_n1_inside"])
    assert not np.array_equal(x[0], x[2]) and l1[0] > 0 and np.array_equal(x[0][:, :3], x[2][:, :3])
    for q in ("empty", "negative", "leaves", "mismatch"):
        x, l1 = sr.statement(by[f"r32_m2_n1_{q}"])
        assert np.array_equal(x[0], x[2]) and l1[0] == 0, q
    assert {c["drawings"].shape[1] for c in CROPS} == {40, 33} and any(list(c["draw"]) != sorted(c["draw"]) for c in CROPS)


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_restated_pairs_equal_the_statement(c):
    x, l1 = OPS.stitch_pairs(*sr.to_torch(c), c["margin"])
    s = c["r"] - 3 * c["margin"]
    assert tuple(x.shape) == (4 * c["n"], 3, s, s) and x.is_contiguous() and l1.dtype == torch.float32
    sr.check_pairs(x.numpy(), l1.numpy(), c)


@pytest.mark.parametrize("c", CROPS, ids=[c["name"] for c in CROPS])
def test_restated_crops_equal_the_statement(c):
    got = OPS.stitch_crops(torch.from_numpy(c["drawings"]), torch.from_numpy(c["draw"]), torch.from_numpy(c["off"]), c["r"])
    want = sr.crop_statement(c)
    assert got.dtype == torch.float32 and got.numpy().tobytes() == want.tobytes()
    # out of range: clamped, as the kernel does
    far = OPS.stitch_crops(torch.from_numpy(c["drawings"]), torch.from_numpy(c["draw"] + np.int32(100)), torch.from_numpy(c["off"] - np.int32(1000)), c["r"])
    k = c["drawings"].shape[0]
    assert np.array_equal(far.numpy()[:, 0], sr.u8_over_255()[c["drawings"][k - 1, :c["r"], :c["r"]]][None].repeat(len(c["draw"]), 0))


def test_restatements_reject_malformed_input():
    c = CASES[0]
    fake, ra, rb = sr.to_torch(c)
    for bad in (lambda: OPS.stitch_pairs(fake[:1], ra, rb, 2), lambda: OPS.stitch_pairs(fake, ra, rb, 11), lambda: OPS.stitch_pairs(fake, ra, rb, -1),
                lambda: OPS.stitch_pairs(fake.double(), ra, rb, 2), lambda: OPS.stitch_pairs(fake, ra.long(), rb, 2),
                lambda: OPS.stitch_pairs(fake, ra[:, :4], rb, 2), lambda: OPS.stitch_pairs(fake[:, :2], ra, rb, 2)):
        with pytest.raises(ValueError):
            bad()
    d = CROPS[0]
    dr, ix, off = torch.from_numpy(d["drawings"]), torch.from_numpy(d["draw"]), torch.from_numpy(d["off"])
    for bad in (lambda: OPS.stitch_crops(dr, ix, off, 41), lambda: OPS.stitch_crops(dr.float(), ix, off, 32), lambda: OPS.stitch_crops(dr, ix.long(), off, 32),
                lambda: OPS.stitch_crops(dr, ix, off[:3], 32), lambda: OPS.stitch_crops(dr[:, :, :39], ix, off, 32)):
        with pytest.raises(ValueError):
            bad()


# ---------------------------------------------------------------------------------------------------------------------
# the reference itself: recorded tensors, CropHelper.composite
# ---------------------------------------------------------------------------------------------------------------------
class _Recorder:
    """Stands where the LPIPS network stands: keeps what it is handed, returns the fixed function the golden's recorder returned."""

    def __init__(self):
        self.x = None

    def pair_distance(self, x):
        self.x = x
        n = x.shape[0] // 2
        return (x[:n] - x[n:]).abs().mean(dim=(1, 2, 3)) * 2 + 1


@pytest.mark.parametrize("margin", [0, 3])
def test_against_the_reference_recording(margin):
    g = load_golden("stitch_metrics.npz")
    assert list(g["margins"]) == [0, 3]
    p = f"m{margin}_"
    n, r = g["fake1"].shape[0], g["fake1"].shape[-1]
    crop1, crop2 = tuple(int(v) for v in g["crop1"]), tuple(int(v) for v in g["crop2"])
    ra, rb = tile_ops.stitch_rects(crop1, crop2, margin)
    assert np.array_equal(ra, sr.crop_pair_rects(crop1, crop2, margin)[0]) and np.array_equal(rb, sr.crop_pair_rects(crop1, crop2, margin)[1])
    fake = torch.from_numpy(np.concatenate([g["fake1"], g["fake2"]]))
    x, l1 = OPS.stitch_pairs(fake, torch.from_numpy(np.repeat(ra[None], n, 0)), torch.from_numpy(np.repeat(rb[None], n, 0)), margin)
    want = np.concatenate([g[p + "lpips_a0"], g[p + "lpips_b0"], g[p + "lpips_a1"], g[p + "lpips_b1"]])
    assert x.numpy().tobytes() == want.tobytes()
    s = r - 3 * margin
    l1_score = 0.5 * (float(l1[:n].sum()) + float(l1[n:].sum())) / (n * 3 * s * s)
    assert abs(l1_score - float(g[p + "STITCH_L1"])) <= 1e-6 * float(g[p + "STITCH_L1"])
    assert np.array_equal(g[p + "positions2"] - g[p + "positions1"], np.repeat(np.array([[crop2[0] - crop1[0], crop2[1] - crop1[1]]]), n, 0))
    # compute_stitching_metrics on the dict of our RandomStitcher: the reference's two numbers
    fakes = [torch.from_numpy(g["fake1"]), torch.from_numpy(g["fake2"])]

    class FakeG:
        img_resolution = r

        def __call__(self, z, c, geom_feature, positions=None, style_mixing_prob=0):
            return fakes.pop(0).clone()
    res = RandomStitcher(margin, int(g["min_overlap"])).generate_with_stitching(FakeG(), torch.zeros(n, 4), None, None, None, crop1, crop2,
                                                                                  positions1=torch.from_numpy(g[p + "positions1"]))
    rec = _Recorder()
    got = metrics.compute_stitching_metrics(res, margin, rec)
    assert list(got) == ["STITCH_LPIPS", "STITCH_L1"] and rec.x.numpy().tobytes() == want.tobytes()
    for key in got:
        assert abs(got[key] - float(g[p + key])) <= 1e-6 * float(g[p + key]), key
    with pytest.raises(ValueError):
        metrics.compute_stitching_metrics(res, 11, rec)


def test_restated_pairs_equal_composite_and_crop_on_random_crops():
    """``CropHelper.composite`` + the crop on crop pairs drawn by ``RandomStitcher`` (input width 100, R = 32)."""
    rng = random.Random(9)
    rs = np.random.RandomState(9)
    r, n = 32, 3
    for margin, min_overlap in ((2, 6), (0, 10), (3, 4), (5, 0)):
        st = RandomStitcher(margin, min_overlap)
        for _ in range(6):
            crop1 = (rng.randint(0, 100 - r), rng.randint(0, 100 - r), r, r)
            crop2 = st.gen_overlapping_square_crop(100, crop1, rng)
            fake = torch.from_numpy(rs.randn(2 * n, 3, r, r).astype(np.float32))
            f1, f2 = fake[:n], fake[n:]
            _, a1, a2 = CropHelper.compute_overlaps(crop1, st.offset_crop(crop2))
            c1 = CropHelper.composite(f1, f2, a1, a2)
            _, a1, a2 = CropHelper.compute_overlaps(st.offset_crop(crop1), crop2)
            c2 = CropHelper.composite(f2, f1, a2, a1)
            crop = lambda t: t[:, :, margin:r - 2 * margin, margin:r - 2 * margin]
            want = torch.cat([crop(f1), crop(f2), crop(c1), crop(c2)])
            ra, rb = tile_ops.stitch_rects(crop1, crop2, margin)
            x, l1 = OPS.stitch_pairs(fake, torch.from_numpy(np.repeat(ra[None], n, 0)), torch.from_numpy(np.repeat(rb[None], n, 0)), margin)
            assert torch.equal(x, want), (margin, crop1, crop2)
            xs, ls = sr.pair_statement(fake.numpy(), np.repeat(ra[None], n, 0), np.repeat(rb[None], n, 0), margin)
            assert xs.tobytes() == x.numpy().tobytes() and np.all(np.abs(l1.numpy() - ls) <= sr.l1_bound(ls, r - 3 * margin))
    # crops that do not overlap: no composite
    ra, rb = tile_ops.stitch_rects((0, 0, r, r), (40, 50, r, r), 2)
    assert not ra.any() and not rb.any()


# ---------------------------------------------------------------------------------------------------------------------
# the plan
# ---------------------------------------------------------------------------------------------------------------------
def test_default_stitch_plan():
    args = dict(seed=4, n_brushes=7, rounds=3, k=5, r=128, d=192, margin=10, min_overlap=50)
    plan, again = metrics.default_stitch_plan(**args), metrics.default_stitch_plan(**args)
    assert sorted(plan) == sorted(metrics.STITCH_PLAN_KEYS)
    assert all(plan[k].dtype == np.int32 and np.array_equal(plan[k], again[k]) for k in plan)
    assert plan["crop1"].shape == (7, 3, 2) and plan["crop2"].shape == (7, 3, 2) and plan["positions1"].shape == (7, 3, 5, 2)
    other = metrics.default_stitch_plan(**dict(args, seed=5))
    assert not np.array_equal(plan["crop1"], other["crop1"])
    radius = 128 - 10 - 50 - 1
    assert plan["crop1"].min() >= 0 and plan["crop1"].max() <= 192 - 128
    lo, hi = np.maximum(0, plan["crop1"] - radius), np.minimum(plan["crop1"] + radius, 192 - 128 - 1)
    assert np.all(plan["crop2"] >= lo) and np.all(plan["crop2"] <= hi)
    assert plan["positions1"].min() >= 0 and plan["positions1"].max() <= 128 - 2
    # a tight geometry: many units, every crop pair overlaps by min_overlap + 1 or more per axis after the inset, in both directions
    tight = metrics.default_stitch_plan(seed=1, n_brushes=40, rounds=2, k=1, r=64, d=200, margin=4, min_overlap=20)
    assert np.abs(tight["crop2"] - tight["crop1"]).max() > 30
    for c1, c2 in zip(tight["crop1"].reshape(-1, 2).tolist(), tight["crop2"].reshape(-1, 2).tolist()):
        a, b = (c1[0], c1[1], 64, 64), (c2[0], c2[1], 64, 64)
        for first, second in ((a, CropHelper.offset_crop(b, 4)), (CropHelper.offset_crop(a, 4), b)):
            ov, a1, a2 = CropHelper.compute_overlaps(first, second)
            assert a1 is not None and ov.min_width >= 21, (c1, c2)
    # the first unit's draws, in the documented order
    gen = torch.Generator().manual_seed(4 + 3)
    c1 = torch.randint(0, 192 - 128 + 1, (2,), generator=gen).tolist()
    assert plan["crop1"][0, 0].tolist() == c1
    for axis in range(2):
        lo, hi = max(0, c1[axis] - radius), min(c1[axis] + radius, 192 - 128 - 1)
        assert int(plan["crop2"][0, 0, axis]) == int(torch.randint(lo, hi + 1, (1,), generator=gen))
    assert np.array_equal(plan["positions1"][0, 0], torch.randint(0, 127, (5, 2), generator=gen).numpy())
    for bad in (dict(d=128), dict(d=100), dict(margin=70, min_overlap=60), dict(min_overlap=118)):
        with pytest.raises(ValueError):
            metrics.default_stitch_plan(**dict(args, **bad))
    assert metrics.default_stitch_plan(**dict(args, min_overlap=117))["crop2"].shape == (7, 3, 2)      # radius 0 is allowed


def test_the_other_streams_are_untouched():
    """``default_colors`` and ``default_crops`` for a seed: the values they had before the stitch plan existed (their own seeds
    ``seed + 1`` and ``seed + 2``, restated here), whether or not a stitch plan is drawn in between."""
    before = metrics.default_colors(3, 2, 2, 4), metrics.default_crops(3, 2, 2, 4, 128, 64)
    metrics.default_stitch_plan(3, 2, 2, 4, 128, 192)
    after = metrics.default_colors(3, 2, 2, 4), metrics.default_crops(3, 2, 2, 4, 128, 64)
    assert np.array_equal(before[0], after[0]) and all(np.array_equal(before[1][k], after[1][k]) for k in before[1])
    gen = torch.Generator().manual_seed(3 + 1)
    assert np.array_equal(before[0][0, 0], torch.rand((4, 3), dtype=torch.float32, generator=gen).numpy())
    gen = torch.Generator().manual_seed(3 + 2)
    assert before[1]["multi_off0"][0, 0].tolist() == torch.randint(0, 128 - 64 + 1, (2,), generator=gen).tolist()


# ---------------------------------------------------------------------------------------------------------------------
# BrushScores and the files
# ---------------------------------------------------------------------------------------------------------------------
def _scores(gold, perceptual_values=None, stitching=None):
    sample = dict(zip(metrics.KEYS, gold["file_sample_values"].tolist()))
    fields = {f: np.array([sample[k], sample[k] / 2], np.float32) for f, k in (("lab_e_percent", "LAB_E%"), ("lab_l2", "LAB_L2"),
                                                                               ("bg_clarity_mean", "BG_CLARITY_MEAN"), ("fg_opacity_median", "FG_OPACITY_MEDIAN"))}
    kw = {} if stitching is None else {"stitching": stitching}
    return metrics.BrushScores(["594", "7"], perceptual=perceptual_values, **fields, **kw)


def test_files_with_and_without_stitching(tmp_path):
    gold = load_golden("brush_metrics.npz")
    assert metrics.STITCH_KEYS == ("STITCH_L1", "STITCH_LPIPS")
    nine = list(metrics.KEYS + metrics.PERCEPTUAL_KEYS + metrics.STITCH_KEYS)
    assert nine == sorted(nine) and len(nine) == 9
    plain = _scores(gold)
    assert plain.stitching is None and [f.name for f in metrics.dataclasses.fields(metrics.BrushScores)][-1] == "stitching"
    style, summary, info = brush_metrics_main.write_scores(plain, str(tmp_path / "a"))
    rows = open(style).read().splitlines(keepends=True)
    assert rows[0] == str(gold["file_style_header"]) and rows[1] == str(gold["file_sample_style_line"]) and len(rows) == 3
    assert open(summary).read().splitlines(keepends=True)[0] == str(gold["file_summary_header"])
    assert list(json.load(open(info))["metrics"]) == list(metrics.KEYS)
    vals = {"LPIPS_ACROSS_GEO": np.array([0.25, 0.5], np.float32), "LPIPS_UNIFORM_BG": np.array([0.125, np.nan], np.float32),
            "LPIPS_UNIFORM_BG_multicolor": np.array([1.5, 0.03125], np.float32)}
    seven = _scores(gold, vals)
    s7 = open(brush_metrics_main.write_scores(seven, str(tmp_path / "b"))[0]).read().splitlines(keepends=True)
    st = {"STITCH_L1": np.array([0.0625, 0.25], np.float32), "STITCH_LPIPS": np.array([0.75, 0.5], np.float32)}
    full = _scores(gold, vals, st)
    style, summary, info = brush_metrics_main.write_scores(full, str(tmp_path / "c"), "p_")
    rows = open(style).read().splitlines(keepends=True)
    assert rows[0] == "SEED            " + metrics.file_line(nine) and rows[0].split() == ["SEED"] + nine
    assert all(r.startswith(o[:-1] + " ") for r, o in zip(rows, s7)) and all(len(r) == len(rows[0]) for r in rows)      # seven columns as before
    assert rows[1].split()[8:] == ["0.0625", "0.7500"] and rows[2].split()[8:] == ["0.2500", "0.5000"]
    top = open(summary).read().splitlines(keepends=True)
    assert top[0] == metrics.file_line(nine) and top[1].split()[7:] == ["0.1562", "0.6250"] and len(top[1]) == len(top[0])
    back = json.load(open(info))
    assert list(back["metrics"]) == nine == list(back["summary"]) == list(full.keys()) == list(full.as_dict())
    assert full.rank("STITCH_L1") == ["594", "7"] and full.rank("STITCH_LPIPS") == ["7", "594"]          # lower is better


def test_parser_takes_the_stitch_arguments():
    base = ["--gan_checkpoint", "e.npz", "--drawings", "d.npz", "--output_dir", "o"]
    a = brush_metrics_main.build_parser().parse_args(base)
    assert (a.stitch_drawings, a.stitch_margin, a.stitch_min_overlap) == (None, 10, 50)
    b = brush_metrics_main.build_parser().parse_args(base + ["--stitch_drawings", "full.npz", "--stitch_margin", "4", "--stitch_min_overlap", "20",
                                                              "--lpips_weights", "w.npz"])
    assert (b.stitch_drawings, b.stitch_margin, b.stitch_min_overlap) == ("full.npz", 4, 20)
    with pytest.raises(SystemExit):                                        # needs --lpips_weights: refused before anything is loaded
        brush_metrics_main.main(base + ["--stitch_drawings", "full.npz"])


# ---------------------------------------------------------------------------------------------------------------------
# the evaluator on the oracle-backed ops
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracle():
    e, g = load_golden("engine_r128.npz"), load_golden("brush_catalogue_r128.npz")
    cfg = cfgmod.style1_config(int(g["resolution"]))
    ops = OracleTileOps(cfg, wmod.random_state_dict(cfg, seed=int(g["weights_seed"])), encmod.random_encoder_state_dict(int(g["encoder_seed"])))
    s = lr.SLIM["alex"]
    w = lr.slim_weights("alex", s["channels"], s["seed"], s["size"])
    full = np.full((2, 192, 192), 255, np.uint8)
    full[:, 20:148, 40:168] = e["uvs_cal_medium"][:2]
    return dict(ops=ops, lib=bc.FixtureLibrary(g, cfg.z_dim), w=w, net=perceptual.LPIPS(w, route="torch", device="cpu"), full=full,
                evaluator=metrics.BrushEvaluator(ops, e["uvs_cal_medium"][:2], seed=br.EVAL_SEED))


def test_evaluator_with_stitch_on_the_oracle_ops(oracle):
    ev, lib, net, w = oracle["evaluator"], oracle["lib"], oracle["net"], oracle["w"]
    ids = lib.get_style_ids()[:2]
    setup = metrics.StitchSetup(oracle["full"], margin=10, min_overlap=50)
    seen, old = [], []

    def hook(units, renders, targets, stitch=None):
        (old if stitch is None else seen).append((list(units), stitch))
    got = ev.evaluate(lib, style_ids=ids, batch=8, lpips=net, stitch=setup, on_pass=hook)
    plain = ev.evaluate(lib, style_ids=ids, batch=8, lpips=net, on_pass=lambda u, r, t: old.append((list(u), None)))
    assert [u for u, _ in seen] == [[(0, 0), (1, 0)]] and [u for u, _ in old] == [[(0, 0), (1, 0)]] * 2
    assert plain.stitching is None and got.keys() == metrics.KEYS + metrics.PERCEPTUAL_KEYS + metrics.STITCH_KEYS
    for key in metrics.KEYS + metrics.PERCEPTUAL_KEYS:                      # the seven other columns: bit for bit
        assert got.as_dict()[key].tobytes() == plain.as_dict()[key].tobytes(), key
    info = seen[0][1]
    plan = metrics.default_stitch_plan(br.EVAL_SEED, 2, 1, 2, 128, 192, 10, 50)
    assert np.array_equal(info["crop1"], plan["crop1"][:, 0]) and np.array_equal(info["crop2"], plan["crop2"][:, 0])
    assert np.array_equal(info["positions1"], plan["positions1"].reshape(4, 2))
    assert np.array_equal(info["positions2"] - info["positions1"], np.repeat(info["crop2"] - info["crop1"], 2, 0))
    fake = info["fake"].numpy()
    assert fake.shape == (8, 3, 128, 128)
    rects = [sr.crop_pair_rects((*info["crop1"][u], 128, 128), (*info["crop2"][u], 128, 128), 10) for u in range(2)]
    ra, rb = (np.repeat(np.stack([q[j] for q in rects]), 2, 0) for j in range(2))
    dist = lambda x: lr.lpips_f64(w, x[:len(x) // 2], x[len(x) // 2:]).numpy()
    want_l1, want_lp = sr.scores_from_fake(fake, ra, rb, 10, 2, dist)
    assert np.all(np.abs(got.stitching["STITCH_L1"] - want_l1) <= sr.l1_bound(want_l1, 98) + sr.EPS32 * want_l1) and np.all(want_l1 > 0)
    assert np.all(np.abs(got.stitching["STITCH_LPIPS"] - want_lp) <= 1e-4 * want_lp) and np.all(want_lp > 0)
    # the first crops of the pass: the windows of the full drawings, encoded and rendered with the plan's positions
    ops = oracle["ops"]
    geo = torch.from_numpy(np.stack([sr.u8_over_255()[oracle["full"][d, y:y + 128, x:x + 128]] for (y, x) in info["crop1"].tolist() for d in range(2)]))[:, None]
    assert np.array_equal(ops.stitch_crops(torch.from_numpy(oracle["full"]), torch.tensor([0, 1, 0, 1], dtype=torch.int32),
                                           torch.from_numpy(np.repeat(info["crop1"], 2, 0).astype(np.int32))).numpy(), geo.numpy())
    empty = ev.evaluate(lib, style_ids=[], lpips=net, stitch=setup)
    assert empty.ids == [] and sorted(empty.stitching) == sorted(metrics.STITCH_KEYS)


def test_evaluate_raises(oracle):
    ev, lib, net = oracle["evaluator"], oracle["lib"], oracle["net"]
    ids = lib.get_style_ids()[:1]
    setup = metrics.StitchSetup(oracle["full"])
    with pytest.raises(ValueError, match="LPIPS"):
        ev.evaluate(lib, style_ids=ids, stitch=setup)
    for bad in (oracle["full"][:, :128, :128], oracle["full"][:, :100, :100], oracle["full"].astype(np.float32), oracle["full"][0], oracle["full"][:, :, :150]):
        with pytest.raises(ValueError):
            ev.evaluate(lib, style_ids=ids, lpips=net, stitch=metrics.StitchSetup(bad))
    with pytest.raises(ValueError):
        ev.evaluate(lib, style_ids=ids, lpips=net, stitch=metrics.StitchSetup(oracle["full"], margin=43))
    with pytest.raises(ValueError):
        ev.evaluate(lib, style_ids=ids, lpips=net, stitch=metrics.StitchSetup(oracle["full"], margin=40, min_overlap=90))
    plan = metrics.default_stitch_plan(0, 1, 1, 2, 128, 192)
    for bad in ({"crop1": plan["crop1"]}, dict(plan, positions1=plan["positions1"][:, :, :1]), dict(plan, crop2=plan["crop2"][0]),
                dict(plan, crop1=plan["crop1"] + 65), dict(plan, crop2=plan["crop2"] - 100)):
        with pytest.raises(ValueError):
            ev.evaluate(lib, style_ids=ids, lpips=net, stitch=setup, stitch_plan=bad)


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

    crops = lambda **kw: lib.nb_stitch_crops_u8(*[{**dict(drawings=a, k=1, d=12, draw=i, off=i, n=1, r=8, out=a, stream=None), **kw}[key] for key in
                                                  ("drawings", "k", "d", "draw", "off", "n", "r", "out", "stream")])
    rejected(crops(drawings=None), "null pointer")
    rejected(crops(off=None), "null pointer")
    rejected(crops(out=None), "null pointer")
    rejected(crops(k=0), "bad sizes")
    rejected(crops(d=7), "bad sizes")
    rejected(crops(r=0), "bad sizes")
    rejected(crops(r=8193, d=9000), "bad sizes")
    rejected(crops(n=-1), "bad sizes")
    rejected(crops(out=a + 2), "4-byte aligned")
    rejected(crops(draw=i + 1), "4-byte aligned")
    rejected(crops(r=8192, d=8192, n=1 << 24), "exceed the grid")
    assert crops(n=0) == 0

    pairs = lambda **kw: lib.nb_stitch_pairs_f32(*[{**dict(fake=a, stride=192, ra=i, rb=i, n=1, r=8, margin=1, out=a, l1=a, partials=a, stream=None), **kw}[key]
                                                   for key in ("fake", "stride", "ra", "rb", "n", "r", "margin", "out", "l1", "partials", "stream")])
    rejected(pairs(fake=None), "null pointer")
    rejected(pairs(rb=None), "null pointer")
    rejected(pairs(l1=None), "null pointer")
    rejected(pairs(partials=None), "null pointer")
    rejected(pairs(r=0), "bad sizes")
    rejected(pairs(n=-1), "bad sizes")
    rejected(pairs(n=(1 << 22) + 1), "bad sizes")
    rejected(pairs(margin=-1), "leaves no crop window")
    rejected(pairs(margin=3), "leaves no crop window")                     # 8 - 9 < 1: the window is R - 3 margin wide, not R - 2 margin
    rejected(pairs(stride=191), "alias")
    rejected(pairs(fake=a + 1), "4-byte aligned")
    rejected(pairs(ra=i + 2), "4-byte aligned")
    assert pairs(n=0) == 0 and pairs(n=0, margin=2) == 0


def test_header_prototypes_and_sources():
    header = open(os.path.join(REPO, "include", "neube_hip.h")).read()
    for name in ("nb_stitch_crops_u8", "nb_stitch_pairs_f32"):
        assert name in _lib.PROTOTYPES and re.search(r"\bint %s\(" % name, header), name
    assert len(_lib.PROTOTYPES["nb_stitch_crops_u8"][1]) == 9 and len(_lib.PROTOTYPES["nb_stitch_pairs_f32"][1]) == 11
    assert re.search(r"#define NB_STITCH_PARTS\s+%d\b" % _lib.NB_STITCH_PARTS, header) and _lib.NB_STITCH_PARTS == sr.PARTS
    for cite in ("geom_metric.py:165-187", "geom_metric.py:173-177", "stitching.py:161-179", "metric_main.py:"):
        assert cite in header, cite
    assert "nb_stitch_metrics.hip" in build.SOURCES and build.FILE_FLAGS["nb_stitch_metrics.hip"] == ["-fno-slp-vectorize"]
    src = open(os.path.join(build.CSRC, "nb_stitch_metrics.hip")).read()
    assert "asymmetric" in src and "atomicAdd" not in src
    assert _lib.ABI_VERSION == 22
    assert sr.chain(226) == 4 * 5 + 40 and sr.chain(26) == 4 + 40
