"""Synthetic drawings without a GPU: the host entry nb_synth_spline_counts against its numpy statement, the properties of the float64
restatements of ``brushstroke_engine_amd.drawings`` (what a CPU device runs and what tests/test_hip_drawings.py holds the kernels to),
the conditions on the scenes and seeds of the GPU tests, the loaders and the command-line tool."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import drawing_refs as R
import philox_ref
import stroke_refs as sr
from brushstroke_engine_amd import _lib, build, brush_metrics_main, drawings as dr, make_drawings_main, painting
from brushstroke_engine_amd.strokes import raster_strokes_numpy

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K_STAT = 4096


def test_source_is_listed_with_the_flags_of_the_stroke_kernels():
    assert "nb_drawings.hip" in build.SOURCES and build.FILE_FLAGS["nb_drawings.hip"] == build.FILE_FLAGS["nb_strokes.hip"]
    assert {"nb_philox.h", "nb_raster_cell.h"} <= set(build.HEADERS)
    header = open(os.path.join(REPO, "include", "neube_hip.h")).read()
    assert int(re.search(r"#define NB_SYNTH_COORD_ROUNDINGS (\d+)", header).group(1)) == _lib.NB_SYNTH_COORD_ROUNDINGS
    assert int(re.search(r"#define NB_SYNTH_MAX_POINTS (\d+)", header).group(1)) == _lib.NB_SYNTH_MAX_POINTS
    assert ctypes.sizeof(_lib.NbSplineSpec) == 8 * 4 + 12 * 4


def test_draws_are_the_seeded_noise_generator():
    """The package's Philox (drawings._draw) is the generator tests/philox_ref.py pins to the Random123 known answers."""
    j, s, seed = np.arange(40, dtype=np.uint64), 0x1234567890ABCDEF, philox_ref.STAT_SEEDS[2]
    want = philox_ref.philox4x32_10((j, dr.SPLN, s & 0xFFFFFFFF, s >> 32), (seed & 0xFFFFFFFF, seed >> 32))
    got = dr._draw(j, np.uint64(s), seed)
    assert all(np.array_equal(a, b) for a, b in zip(got, want))


# ---------------------------------------------------------------------------------------------------------------------
# counts
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", philox_ref.STAT_SEEDS)
def test_counts_entry_equals_numpy(seed):
    spec = dr.SplineSpec()
    synth = dr.SplineSynth(spec, 256, seed)
    got = synth.counts(K_STAT, offset=3)
    want = dr.synth_counts_numpy(spec, seed, 3, K_STAT)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    assert sorted(set(got.tolist())) == list(range(spec.pts_min, spec.pts_max + 1))          # every value occurs
    # drawing k at offset o is drawing 0 at offset o + k, also across the 64-bit wrap
    for k in (1, 77, K_STAT - 1):
        assert synth.counts(1, offset=3 + k)[0] == got[k]
    top = (1 << 64) - 2
    assert np.array_equal(synth.counts(4, offset=top), np.concatenate([synth.counts(2, offset=top), synth.counts(2, offset=0)]))
    assert np.array_equal(synth.counts(4, offset=top), dr.synth_counts_numpy(spec, seed, top, 4))


def test_counts_entry_validates():
    lib = _lib.lib()
    out = np.zeros(4, np.int32)
    good = dr.SplineSpec().to_c()
    assert lib.nb_synth_spline_counts(ctypes.addressof(good), 1, 0, 4, out.ctypes.data) == 0
    assert lib.nb_synth_spline_counts(None, 1, 0, 4, out.ctypes.data) == _lib.NB_EINVAL
    assert lib.nb_synth_spline_counts(ctypes.addressof(good), 1, 0, 4, None) == _lib.NB_EINVAL
    for field, value in (("pts_min", 3), ("pts_max", 65), ("mode", 2), ("thick_mode", 3), ("n_mix", 5)):
        bad = dr.SplineSpec().to_c()
        setattr(bad, field, value)
        assert lib.nb_synth_spline_counts(ctypes.addressof(bad), 1, 0, 4, out.ctypes.data) == _lib.NB_EINVAL, field
    bad = dr.SplineSpec().to_c()
    bad.cdf[1] = 0.5                                                        # the last cumulative weight must be 1
    assert lib.nb_synth_spline_counts(ctypes.addressof(bad), 1, 0, 4, out.ctypes.data) == _lib.NB_EINVAL
    assert b"cdf" in lib.nb_last_error()
    # the device entries validate on the host before any launch: usable without a GPU
    assert lib.nb_synth_spline_ctrl_f32(ctypes.addressof(good), 1, 0, 4, 64, None, None, 16, None) == _lib.NB_EINVAL
    assert lib.nb_raster_batch_u8(None, None, 0, 1, None, 8, 8, 0, 0, None) == _lib.NB_EINVAL
    with pytest.raises(ValueError, match="pts"):
        dr.SplineSpec(pts_min=3)


# ---------------------------------------------------------------------------------------------------------------------
# control points and thickness
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [64, 256])
def test_cells_mode_uses_distinct_cells(r):
    spec = dr.SplineSpec(mode="cells", pts_min=4, pts_max=20).scaled(r)
    ctrl, off = dr.synth_ctrl_numpy(spec, 2, 0, 256, r)
    assert off[0] == 0 and off[-1] == ctrl.shape[0] and np.array_equal(np.diff(off), dr.synth_counts_numpy(spec, 2, 0, 256))
    beyond = 0
    for d in range(256):
        rows = ctrl[off[d]:off[d + 1]]
        first = rows[:16]
        assert (first[:, :2] >= 0).all() and (first[:, :2] < r).all()                      # inside the grid, so inside their cell
        cells = R.cells_of(first, r)
        assert len(set(cells.tolist())) == len(first)
        rest = rows[16:, :2]
        assert (rest >= -0.05 * r - 1e-4).all() and (rest < 1.05 * r + 1e-4).all()
        beyond += len(rest)
    assert beyond > 0
    # a drawing of 16 points or more takes every cell exactly once
    full = [d for d in range(256) if off[d + 1] - off[d] >= 16]
    assert full and all(sorted(R.cells_of(ctrl[off[d]:off[d] + 16], r).tolist()) == list(range(16)) for d in full)


@pytest.mark.parametrize("r", [64, 256])
def test_uniform_mode_range(r):
    ctrl, _ = dr.synth_ctrl_numpy(dr.SplineSpec().scaled(r), 5, 0, 512, r)
    assert (ctrl[:, :2] >= 0).all() and (ctrl[:, :2] < 1.1 * r).all()
    assert ctrl[:, :2].max() > 1.05 * r and ctrl[:, :2].min() < 0.05 * r                    # the range is used


@pytest.mark.parametrize("seed", philox_ref.STAT_SEEDS)
def test_mixture_thickness_statistics(seed):
    """Radii are non-negative integers, and their mean over 4096 draws is within five standard errors of the mixture's.
    With p = weights / sum: mean = sum p mu, variance = sum p (sigma^2 + mu^2) - mean^2, plus 1/12 for the rounding to integers.
    The truncation at -0.5 (a redraw, up to eight times) moves a component's mean by sigma phi(a) / (1 - Phi(a)) with
    a = (-0.5 - mu) / sigma: a = -3.25 and -3.5 for the default mixture, i.e. 2 * 0.0020 * 0.375 + 3 * 0.00087 * 0.625 = 0.003 in all,
    against a bound of 5 * sqrt(10.96 / 4096) = 0.26."""
    spec = dr.SplineSpec()
    radii = dr.synth_radii_numpy(spec, seed, 0, K_STAT)
    assert (radii >= 0).all() and np.array_equal(radii, np.rint(radii))
    p = np.asarray(spec.weights) / sum(spec.weights)
    mu, sg = np.asarray(spec.centers), np.asarray(spec.sigmas)
    mean = float((p * mu).sum())
    var = float((p * (sg ** 2 + mu ** 2)).sum()) - mean ** 2 + 1.0 / 12.0
    bound = 5.0 * math.sqrt(var / K_STAT)
    shift = sum(pc * s * math.exp(-0.5 * a * a) / math.sqrt(2 * math.pi) / (1 - 0.5 * math.erfc(-a / math.sqrt(2)))
                for pc, m, s in zip(p, mu, sg) for a in [(-0.5 - m) / s])
    assert shift < 0.02 * bound
    assert abs(radii.mean() - mean) <= bound, (radii.mean(), mean, bound)
    # both components are drawn, in the proportion of the weights (five standard errors of a share)
    c = np.searchsorted(spec.cdf().astype(np.float64), dr._unit(dr._draw(0, dr._samples(0, K_STAT), seed)[1]), side="right")
    assert abs((c == 0).mean() - p[0]) <= 5.0 * math.sqrt(p[0] * p[1] / K_STAT)
    # r_eff: the radius from 2 up, half a pixel below
    ctrl, off = dr.synth_ctrl_numpy(spec, seed, 0, 64, 256)
    assert np.array_equal(ctrl[off[:-1], 2], np.where(radii[:64] >= 2, radii[:64], 0.5))


def test_range_and_fixed_thickness_and_rejection():
    spec = dr.SplineSpec(thick="range", rmin=1, rmax=6)
    radii = dr.synth_radii_numpy(spec, 1, 0, 512)
    assert sorted(set(radii.tolist())) == [1, 2, 3, 4, 5, 6]
    assert (dr.synth_radii_numpy(dr.SplineSpec().fixed(7), 1, 0, 9) == 7).all()
    # a mixture that is never accepted gives radius 0 (eight tries, then none), so r_eff 0.5
    never = dr.SplineSpec(centers=(-50.0,), sigmas=(1.0,), weights=(1.0,))
    assert (dr.synth_radii_numpy(never, 1, 0, 32) == 0).all()
    assert (dr.synth_ctrl_numpy(never, 1, 0, 4, 64)[0][:, 2] == 0.5).all()


def test_scaled_spec():
    s = dr.SplineSpec(thick="range").scaled(64)
    assert (s.rmin, s.rmax, s.centers, s.sigmas) == (1, 8, (1.5, 2.5), (0.5, 0.75))
    assert dr.SplineSpec().scaled(256) == dr.SplineSpec()
    assert dr.SplineSpec().fixed(16).scaled(128).radius == 8.0


# ---------------------------------------------------------------------------------------------------------------------
# raster
# ---------------------------------------------------------------------------------------------------------------------
def test_raster_batch_numpy_equals_per_drawing_raster():
    synth = dr.SplineSynth(R.e2e_spec(), R.E2E_R, R.E2E_SEED)
    got = synth.batch(R.E2E_K).numpy()
    assert got.shape == (R.E2E_K, R.E2E_R, R.E2E_R) and got.dtype == np.uint8 and set(np.unique(got)) == {0, 255}
    for i in range(R.E2E_K):
        strokes = synth.strokes(i)
        assert strokes.items[0]["through_ends"] is False
        assert np.array_equal(got[i], raster_strokes_numpy(strokes, (R.E2E_R, R.E2E_R))), i
        assert np.array_equal(got[i], raster_strokes_numpy(painting.StrokeList.from_json(strokes.to_json()), (R.E2E_R, R.E2E_R))), i
    # any batch size: 8 = 3 ++ 5
    assert np.array_equal(got, np.concatenate([synth.batch(3).numpy(), synth.batch(5, offset=3).numpy()]))
    # the ops' numpy route
    ops = painting.TileOpsBase()
    lists = [synth.strokes(i) for i in range(3)] + [sr.e2e_strokes()]
    both = ops.raster_strokes_batch(lists, (70, 66), (3, -5))
    assert both.shape == (4, 70, 66) and all(torch.equal(both[i], ops.raster_strokes(lists[i], (70, 66), (3, -5))) for i in range(4))


def test_pairs_share_their_curves():
    synth = dr.SplineSynth(R.e2e_spec(), R.E2E_R, 4)
    medium, thick = (t.numpy() for t in synth.pairs(4, (2, 5)))
    assert ((thick == 0) | (medium == 255)).all() and (thick == 0).sum() > (medium == 0).sum()       # thick covers medium
    a, _ = synth.control(4, 0, synth.spec.fixed(2))
    b, _ = synth.control(4, 0, synth.spec.fixed(5))
    assert torch.equal(a[:, :2], b[:, :2]) and (a[:, 2] == 2).all() and (b[:, 2] == 5).all()


def test_clipping_leaves_the_next_drawing_untouched():
    case = next(c for c in R.batch_cases() if c["name"] == "k2-clipping")
    got = dr.raster_batch_numpy(case["segs"], case["seg_off"], (case["h"], case["w"]), case["off"])
    assert (got[1] == 255).all()
    assert (got[0][-1] == 0).any() and (got[0][:, -1] == 0).any() and (got[0][0] == 0).any()         # it leaves through three edges
    sr.check_raster(got[0], R.drawing_rows(case, 0), case["off"])


@pytest.mark.parametrize("case", R.batch_cases(), ids=lambda c: c["name"])
def test_batch_scenes_keep_the_band_cap(case):
    for i in range(case["k"]):
        share = sr.band_share(R.case_margin(case, i))
        assert share <= (0.0 if case["exact"] else sr.BAND_CAP), (i, share)
    got = dr.raster_batch_numpy(case["segs"], case["seg_off"], (case["h"], case["w"]), case["off"])
    for i in range(case["k"]):
        sr.check_raster(got[i], R.drawing_rows(case, i), case["off"], exact=case["exact"])


def test_synthetic_scenes_keep_the_band_cap():
    """The end-to-end drawings of the GPU test, on the rows of the CPU route (float64 flattening of the float32 control points; the
    device's rows differ from them by fp32 rounding, and the GPU test checks the share again on the rows it read)."""
    synth = dr.SplineSynth(R.e2e_spec(), R.E2E_R, R.E2E_SEED)
    segs, seg_off = synth.segments(R.E2E_K)
    for i in range(R.E2E_K):
        assert sr.band_share(sr.margin64(segs.numpy()[seg_off[i]:seg_off[i + 1]], R.E2E_R, R.E2E_R)) <= sr.BAND_CAP


def test_gpu_seeds_keep_clear_of_the_boundaries():
    """No thickness try the GPU tests evaluate has v within 1e-3 of a half-integer in float64: the rounding boundaries of rintf and
    the acceptance boundary -0.5, where fp32 and float64 may part."""
    for r in R.CTRL_SIDES:
        for name, spec in R.ctrl_specs(r).items():
            if spec.thick == "mixture":
                v = R.evaluated_tries(spec, R.CTRL_SEEDS[r], R.CTRL_OFFSET, R.CTRL_K)
                assert len(v) >= R.CTRL_K and R.half_distance(v).min() >= R.HALF_MARGIN, (r, name, R.half_distance(v).min())
    v = R.evaluated_tries(R.e2e_spec(), R.E2E_SEED, 0, R.E2E_K)
    assert R.half_distance(v).min() >= R.HALF_MARGIN
    assert R.coord_bound(64) == 3 * 2.0 ** -17 and R.coord_bound(256) == 3 * 2.0 ** -15


# ---------------------------------------------------------------------------------------------------------------------
# loaders and the command-line tool
# ---------------------------------------------------------------------------------------------------------------------
def test_synth_forms_parse():
    k, seed, spec, radii, size = dr.parse_synth("synth:4", 64)
    assert (k, seed, radii, size) == (4, 0, None, 64) and spec == dr.SplineSpec().scaled(64)
    assert dr.parse_synth("synth:4:9", 64)[:2] == (4, 9)
    k, seed, spec, radii, size = dr.parse_synth("synth:2:1:mode=cells,pts=5-9,thick=rand,size=200", 64)
    assert (spec.mode, spec.pts_min, spec.pts_max, spec.thick, spec.rmin, spec.rmax, size) == ("cells", 5, 9, "range", 1, 8, 200)
    spec = dr.parse_synth("synth:2::thick=2-6", 64)[2]
    assert (spec.thick, spec.rmin, spec.rmax) == ("range", 2, 6)                               # given in pixels: not scaled
    assert dr.parse_synth("synth:2:1:thick=gauss", 128)[2].centers == (3.0, 5.0)
    assert dr.parse_synth("synth:3:1:radii=3/5", 64)[3] == [3, 5]
    for bad, word in (("synth:", "synth:K"), ("synth:x", "K"), ("synth:0", "K"), ("synth:2:s", "seed"), ("synth:2:1:colour=3", "colour"),
                      ("synth:2:1:mode=grid", "mode"), ("synth:2:1:pts=5", "pts"), ("synth:2:1:pts=2-9", "pts"), ("synth:2:1:radii=a", "radii"),
                      ("synth:2:1:thick=fat", "thick"), ("synth:2:1:size=64", "size"), ("synth:2:1:size=", "size")):
        with pytest.raises(ValueError, match=re.escape(word)):
            dr.parse_synth(bad, 64)
    with pytest.raises(ValueError, match="synth"):
        dr.load_calibration("synth:1:2", 64)


def test_load_drawings_synth_and_path(tmp_path):
    got = dr.load_drawings("synth:3:2:mode=cells", 64)
    assert got.shape == (3, 64, 64) and got.dtype == np.uint8
    assert np.array_equal(got, dr.SplineSynth(dr.SplineSpec(mode="cells").scaled(64), 64, 2).batch(3).numpy())
    assert np.array_equal(brush_metrics_main.load_drawings("synth:3:2:mode=cells", 64), got)
    big = dr.load_drawings("synth:2:1:size=96,thick=2-3", 64)
    assert big.shape == (2, 96, 96)
    cyc = dr.load_drawings("synth:4:2:radii=2/5,mode=cells", 64)
    synth = dr.SplineSynth(dr.SplineSpec(mode="cells").scaled(64), 64, 2)
    assert np.array_equal(cyc[1], synth.batch(1, 1, synth.spec.fixed(5)).numpy()[0])
    assert np.array_equal(cyc[2], synth.batch(1, 2, synth.spec.fixed(2)).numpy()[0])
    # a path: what the reader of the brush tools has always returned
    path, first = str(tmp_path / "d.npz"), str(tmp_path / "first.npz")
    np.savez(path, other=np.zeros(3), drawings=got.astype(np.int32))
    np.savez(first, stuff=got)
    for p in (path, first):
        back = dr.load_drawings(p, 64, "cpu")
        assert back.dtype == np.uint8 and np.array_equal(back, got) and np.array_equal(brush_metrics_main.load_drawings(p), got)
    cal = str(tmp_path / "cal.npz")
    np.savez(cal, medium=got[:2], thick=got[1:])
    m, t = dr.load_calibration(cal)
    assert np.array_equal(m, got[:2]) and np.array_equal(t, got[1:])


class _CalibrationOps(painting.TileOpsBase):
    """What StyleUVSMapper.set_calibration asks of its ops, on the host."""
    patch_width = 64

    def to_device(self, a):
        return torch.from_numpy(np.ascontiguousarray(a))

    def encode(self, geom):
        return [geom]


def test_synth_calibration_passes_set_calibration():
    medium, thick = dr.load_calibration("synth:2", 64)
    assert medium.shape == thick.shape == (5, 64, 64) and medium.dtype == thick.dtype == np.uint8
    assert ((thick == 255).reshape(5, -1).sum(axis=1) >= painting.StyleUVSMapper.TOP_K).all()
    assert ((thick == 0) | (medium == 255)).all()
    mapper = painting.StyleUVSMapper(_CalibrationOps(), medium, thick)
    assert mapper.bmask.shape == (5, 1, 64, 64) and mapper.geom_feature[0].shape == (5, 1, 64, 64)
    again = dr.load_calibration("synth:2", 64)
    assert np.array_equal(again[0], medium) and not np.array_equal(dr.load_calibration("synth", 64)[0], medium)
    # a demand no drawing meets: the retries are bounded
    with pytest.raises(RuntimeError, match="background"):
        dr.load_calibration("synth:2", 64, min_background=64 * 64 + 1)
    # one that only some meet: those that do not are drawn again at the next offsets
    need = int(np.sort((thick == 255).reshape(5, -1).sum(axis=1))[2])
    m2, t2 = dr.load_calibration("synth:2", 64, min_background=need)
    kept = (thick == 255).reshape(5, -1).sum(axis=1) >= need
    assert 0 < kept.sum() < 5 and np.array_equal(t2[kept], thick[kept]) and ((t2 == 255).reshape(5, -1).sum(axis=1) >= need).all()


def test_make_drawings_main(tmp_path):
    out, pngs = str(tmp_path / "sub" / "drawings.npz"), str(tmp_path / "png")
    args = ["--samples", "3", "--width", "64", "--out", out, "--seed", "5", "--smart_sampling", "--device", "cpu"]
    assert make_drawings_main.main(args + ["--png_dir", pngs]) == out
    back = brush_metrics_main.load_drawings(out)
    spec = dr.SplineSpec(mode="cells").scaled(64)
    assert np.array_equal(back, dr.SplineSynth(spec, 64, 5).batch(3).numpy())
    with np.load(out) as z:
        radii = z["radii"]
        assert np.array_equal(radii, dr.synth_radii_numpy(spec, 5, 0, 3).astype(np.int32)) and "medium" not in z.files
    from PIL import Image
    names = sorted(os.listdir(pngs))
    assert names == ["spline%06d_rad%03d.png" % (i, radii[i]) for i in range(3)]
    assert np.array_equal(np.asarray(Image.open(os.path.join(pngs, names[1]))), back[1])
    # --use_radii with two radii: the calibration file
    cal = str(tmp_path / "cal.npz")
    make_drawings_main.main(["--samples", "2", "--width", "64", "--out", cal, "--use_radii", "3", "6", "--device", "cpu", "--thick_dist", "rand",
                             "--png_dir", pngs])
    m, t = dr.load_calibration(cal)
    synth = dr.SplineSynth(dr.SplineSpec().scaled(64), 64, 0)
    want = synth.pairs(2, (3, 6))
    assert np.array_equal(m, want[0].numpy()) and np.array_equal(t, want[1].numpy())
    assert np.array_equal(brush_metrics_main.load_drawings(cal), np.stack([m[0], t[0], m[1], t[1]]))
    assert {"spline000001_rad003.png", "spline000001_rad006.png"} <= set(os.listdir(pngs))
    with pytest.raises(SystemExit):
        make_drawings_main.main(["--samples", "2", "--out", cal, "--pts_min", "2"])
