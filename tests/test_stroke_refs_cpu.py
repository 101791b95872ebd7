"""Vector strokes, the parts that need no GPU: the float64 restatements (tests/stroke_refs.py) against the reference's recorded
spline samples, the numpy route of ``painting`` against them, ``StrokeList``, the host-side argument checks of the three entries of
``csrc/nb_strokes.hip``, ``paint_strokes`` on the oracle-backed ops against the host route ``paint_image``, the ``--strokes``
arguments of ``paint_image_main`` -- and the band condition the device tests rely on, checked here on the reference alone."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

import compose_refs as cr
import stroke_refs as sr
from conftest import load_golden
from brushstroke_engine_amd import _lib, build, paint_image_main, painting

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("nb_raster_segments_u8", "nb_spline_flatten_f32", "nb_spline_segment_count")

# tests/golden/make_golden_spline.py, largest |reference - float64 restatement| over all recorded samples, relative to the control
# sets' coordinate extent.  The reference computes in float32 (control points, knots and the pyramid), so this is its rounding.
MEASURED_REL_DEV = 4.173e-07


@pytest.fixture(scope="module")
def library():
    build.build()
    return _lib.lib()


# ---------------------------------------------------------------------------------------------------------------------
# the spline restatement against the reference's samples
# ---------------------------------------------------------------------------------------------------------------------
def test_spline_restatement_reproduces_the_reference_samples():
    g = load_golden("spline_samples.npz")
    names = [str(n) for n in g["names"]]
    assert len(names) >= 5 and {g[f"{n}_ctrl"].shape[0] for n in names} >= {4, 9}
    assert abs(float(g["max_rel_dev"]) - MEASURED_REL_DEV) <= 1e-3 * MEASURED_REL_DEV          # the noted figure is the fixture's
    worst = 0.0
    for n in names:
        ctrl, ts, t, idx, pts = (g[f"{n}_{k}"] for k in ("ctrl", "ts", "t", "idx", "pts"))
        extent = float(np.ptp(ctrl, axis=0).max())
        mine = sr.knots(ctrl)
        assert np.abs(mine - ts).max() <= 1e-6 * ts[-1], n                                    # float32 running sums of a few terms
        got = np.stack([sr.sample(ctrl, tv, int(i)) for tv, i in zip(t, idx)])
        dev = float(np.abs(got - pts).max()) / extent
        print(f"{n}: max deviation / extent = {dev:.3e}")
        worst = max(worst, dev)
    assert worst <= 4 * MEASURED_REL_DEV
    assert worst < 1e-4                       # anything larger is a wrong formula, not rounding


def test_spline_passes_through_its_inner_control_points():
    ctrl = load_golden("spline_samples.npz")["nine_ctrl"].astype(np.float64)
    ts = sr.knots(ctrl)
    for i in range(ctrl.shape[0] - 3):                      # span i runs from control point i + 1 (t1) to i + 2 (t2)
        assert np.abs(sr.sample(ctrl, ts[i + 1], i) - ctrl[i + 1]).max() < 1e-9
        assert np.abs(sr.sample(ctrl, ts[i + 2], i) - ctrl[i + 2]).max() < 1e-9


@pytest.mark.parametrize("n_strokes,subdiv", [(1, 1), (2, 8), (5, 8), (5, 1)])
def test_numpy_flatten_equals_the_restatement(n_strokes, subdiv):
    ctrl, off = sr.spline_scene(n_strokes, seed=7 + n_strokes)
    a = painting.flatten_splines_numpy(ctrl, off, subdiv)
    b = sr.flatten(ctrl, off, subdiv)
    assert a.shape == b.shape == (sr.segment_count(off, subdiv), 5)
    assert np.abs(a - b).max() <= 1e-12 * 128
    for s in range(n_strokes):                              # watertight, and at the closed-form offsets
        r0, r1 = (int(off[s]) - 3 * s) * subdiv, (int(off[s + 1]) - 3 * (s + 1)) * subdiv
        assert np.array_equal(a[r0 + 1:r1, :2], a[r0:r1 - 1, 2:4])
        assert np.abs(a[r0, :2] - ctrl[off[s] + 1, :2]).max() < 1e-9 and np.abs(a[r1 - 1, 2:4] - ctrl[off[s + 1] - 2, :2]).max() < 1e-9


# ---------------------------------------------------------------------------------------------------------------------
# the band condition of the device tests, on the reference alone
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sr.raster_cases(), ids=lambda c: c[0])
def test_band_condition_of_the_raster_scenes(case):
    """Pixels with |margin64| < 1e-3 are excluded from the device comparison: at most 0.2 % of an image, none for the exact
    scenes.  (Twelve random polylines of 5 segments with fractional coordinates and radii 0.5-6 on 256 x 256 had 0.01-0.05 %.)"""
    name, segs, h, w, off, exact = case
    share = sr.band_share(sr.case_margin(case))
    print(f"{name}: {share * 100:.4f} % of {h * w} pixels in the band")
    assert share <= (0.0 if exact else sr.BAND_CAP)


def test_band_condition_of_the_spline_and_end_to_end_scenes():
    for n_strokes, subdiv in [(1, 1), (2, 8), (5, 8), (5, 1)]:
        ctrl, off = sr.spline_scene(n_strokes, seed=7 + n_strokes)
        segs = sr.flatten(ctrl, off, subdiv, dtype=np.float32)          # (the device's own rows are checked again on the GPU)
        assert sr.band_share(sr.margin64(segs, 130, 130, (3, 2))) <= sr.BAND_CAP
    strokes = sr.e2e_strokes()
    ctrl, off = strokes.spline_control()
    segs = np.concatenate([strokes.polyline_segments()[:, :5], sr.flatten(ctrl, off, 8, dtype=np.float32)])
    assert sr.band_share(sr.margin64(segs, *sr.E2E_SIZE)) <= sr.BAND_CAP


def test_dead_rows_have_no_margin():
    rows = sr.dead_rows()
    assert not sr.valid_rows(rows).any() and np.isinf(sr.margin64(rows, 40, 40)).all()
    assert (painting.raster_segments_numpy(rows, (40, 40)) == 255).all()


# ---------------------------------------------------------------------------------------------------------------------
# the numpy route
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("off", [(0, 0), (10, 10)])
def test_raster_strokes_numpy_equals_margin(off):
    strokes = sr.e2e_strokes()
    h, w = sr.E2E_SIZE[0] + 2 * off[0], sr.E2E_SIZE[1] + 2 * off[1]
    got = painting.raster_strokes_numpy(strokes, (h, w), off, subdiv=8)
    ctrl, so = strokes.spline_control()
    segs = np.concatenate([strokes.polyline_segments()[:, :5].astype(np.float64), sr.flatten(ctrl, so, 8)])
    m = sr.margin64(segs, h, w, off)
    assert got.dtype == np.uint8 and np.array_equal(got, np.where(m <= 0, 0, 255))
    assert 0 < (got == 0).mean() < 0.2


def test_raster_segments_numpy_equals_margin_on_the_scenes():
    for case in sr.raster_cases():
        name, segs, h, w, off, _ = case
        assert np.array_equal(painting.raster_segments_numpy(segs, (h, w), off), np.where(sr.case_margin(case) <= 0, 0, 255)), name


# ---------------------------------------------------------------------------------------------------------------------
# StrokeList
# ---------------------------------------------------------------------------------------------------------------------
def test_stroke_list_json_round_trip():
    s = sr.e2e_strokes()
    s.add_spline([[1, 2], [3, 4], [9, 9], [12, 3]], 1.5, through_ends=False)
    text = s.to_json()
    data = json.loads(text)
    assert [d["type"] for d in data] == ["spline", "spline", "polyline", "polyline", "spline"]
    assert all(set(d) <= {"type", "points", "radius", "through_ends"} for d in data) and data[-1]["through_ends"] is False
    assert isinstance(data[0]["radius"], float) and isinstance(data[1]["radius"], list)
    back = painting.StrokeList.from_json(text)
    assert back.to_json() == text and len(back) == len(s) == 5
    assert np.array_equal(back.polyline_segments(), s.polyline_segments())
    for a, b in zip(back.spline_control(), s.spline_control()):
        assert np.array_equal(a, b)
    assert np.array_equal(painting.StrokeList.from_json(data).polyline_segments(), s.polyline_segments())
    with pytest.raises(ValueError):
        painting.StrokeList.from_json('[{"type": "circle", "points": [[0, 0]], "radius": 1}]')


def test_stroke_list_polyline_radii():
    s = painting.StrokeList().add_polyline([[0, 0], [10, 0], [10, 5]], [1, 3, 2]).add_polyline([[4, 4], [6, 7]], 2.5).add_polyline([[1, 1]], 2)
    rows = s.polyline_segments()
    assert rows.shape == (4, painting.SEG_PITCH) and rows.dtype == np.float32 and (rows[:, 5:] == 0).all()
    assert np.array_equal(rows[:, :5], np.array([[0, 0, 10, 0, 2], [10, 0, 10, 5, 2.5], [4, 4, 6, 7, 2.5], [1, 1, 1, 1, 2]], np.float32))
    for bad in (dict(points=[[0, 0, 0]], radius=1), dict(points=[[0, 0], [1, 1]], radius=[1, 2, 3]), dict(points=[[0, 0]], radius=-1),
                dict(points=[[0, np.nan]], radius=1)):
        with pytest.raises(ValueError):
            painting.StrokeList().add_polyline(**bad)


def test_stroke_list_spline_ends_duplicates_and_radii():
    pts = [[10, 10], [40, 30], [40, 30], [80, 20], [120, 60], [120, 60], [120, 60]]
    rad = [1, 2, 2, 3, 4, 4, 4]
    s = painting.StrokeList().add_spline(pts, rad)
    ctrl, off = s.spline_control()
    assert list(off) == [0, 6] and ctrl.dtype == np.float32                       # 4 distinct points + 2 phantom ends
    assert np.array_equal(ctrl[1:-1], np.array([[10, 10, 1], [40, 30, 2], [80, 20, 3], [120, 60, 4]], np.float32))
    assert np.array_equal(ctrl[0, :2], [2 * 10 - 40, 2 * 10 - 30]) and np.array_equal(ctrl[-1, :2], [2 * 120 - 80, 2 * 60 - 20])
    segs = painting.flatten_splines_numpy(ctrl, off, 8)
    assert segs.shape == (3 * 8, 5) and np.isfinite(segs).all() and s.spline_segment_count(8) == 24
    assert np.abs(segs[0, :2] - [10, 10]).max() < 1e-9 and np.abs(segs[-1, 2:4] - [120, 60]).max() < 1e-9      # through the ends
    assert np.allclose(segs[:8, 4], 1 + (np.arange(8) + 0.5) / 8) and np.allclose(segs[16:, 4], 3 + (np.arange(8) + 0.5) / 8)
    # without the phantom ends the curve runs between the inner points only, and needs four of them
    s2 = painting.StrokeList().add_spline(pts, rad, through_ends=False)
    c2, o2 = s2.spline_control()
    assert np.array_equal(c2, ctrl[1:-1]) and list(o2) == [0, 4]
    f2 = painting.flatten_splines_numpy(c2, o2, 4)
    assert np.abs(f2[0, :2] - [40, 30]).max() < 1e-9 and np.abs(f2[-1, 2:4] - [80, 20]).max() < 1e-9
    with pytest.raises(ValueError):
        painting.StrokeList().add_spline([[0, 0], [1, 1], [1, 1]], 1, through_ends=False)
    with pytest.raises(ValueError):
        painting.StrokeList().add_spline([[3, 3], [3, 3]], 1)
    # the keep-the-duplicate case: a repeated control point has zero knot intervals and yields non-finite rows
    dup = np.array([[0, 0, 1], [10, 0, 1], [10, 0, 1], [20, 5, 1], [30, 5, 1]], np.float32)
    assert not np.isfinite(painting.flatten_splines_numpy(dup, np.array([0, 5], np.int32), 2)[:, :4]).any()


# ---------------------------------------------------------------------------------------------------------------------
# the C entries: argument checks on the host, header / binding agreement
# ---------------------------------------------------------------------------------------------------------------------
def test_entries_validate_on_the_host(library):
    """Bad arguments are refused before any launch (no GPU needed); the pointers are never dereferenced on the host."""
    p = 0x1000
    ok = dict(segs=p, n=4, out=p, h=8, w=8, oy=0, ox=0, clear=1)

    def raster(**kw):
        a = dict(ok, **kw)
        return library.nb_raster_segments_u8(a["segs"], a["n"], a["out"], a["h"], a["w"], a["oy"], a["ox"], a["clear"], None)
    for bad in (dict(segs=None), dict(out=None), dict(n=-1), dict(h=0), dict(w=0), dict(h=-3), dict(h=1 << 16, w=1 << 15),
                dict(h=46341, w=46341), dict(clear=2), dict(clear=-1), dict(segs=p + 4)):
        assert raster(**bad) == _lib.NB_EINVAL, bad
        assert library.nb_last_error()
    assert raster(n=0, clear=0, segs=None) == _lib.NB_OK                 # nothing to draw and nothing to fill: no launch at all

    okf = dict(ctrl=p, off=p, pts=9, ns=2, sub=8, alpha=0.5, segs=p, cap=24)

    def flat(**kw):
        a = dict(okf, **kw)
        return library.nb_spline_flatten_f32(a["ctrl"], a["off"], a["pts"], a["ns"], a["sub"], a["alpha"], a["segs"], a["cap"], None)
    for bad in (dict(ctrl=None), dict(off=None), dict(segs=None), dict(ns=0), dict(ns=-1), dict(sub=0), dict(pts=7), dict(cap=23),
                dict(cap=0), dict(alpha=-0.5), dict(alpha=float("nan")), dict(alpha=1.5), dict(segs=p + 8),
                dict(pts=(1 << 31) - 1, ns=1, sub=2, cap=(1 << 31) - 1)):
        assert flat(**bad) == _lib.NB_EINVAL, bad
    assert b"capacity" in (flat(cap=23), library.nb_last_error())[1]


def test_segment_count_matches_python(library):
    for pts, ns, sub in [(4, 1, 1), (4, 1, 8), (9, 1, 8), (13, 2, 3), (40, 5, 8), (0, 0, 8), (1 << 30, 7, 64)]:
        assert library.nb_spline_segment_count(pts, ns, sub) == (pts - 3 * ns) * sub
    for pts, ns, sub in [(3, 1, 8), (7, 2, 8), (8, 2, 0), (8, -1, 1)]:
        assert library.nb_spline_segment_count(pts, ns, sub) == _lib.NB_EINVAL
    s = sr.e2e_strokes()
    ctrl, off = s.spline_control()
    assert library.nb_spline_segment_count(ctrl.shape[0], len(off) - 1, 8) == s.spline_segment_count(8) == sr.segment_count(off, 8) \
        == painting.flatten_splines_numpy(ctrl, off, 8).shape[0]


def test_header_and_binding_agree_on_the_entries(library):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "neube_hip.h")).read(), flags=re.S)
    ctype = {"int": C.c_int, "float": C.c_float, "void*": C.c_void_p, "const float*": C.c_void_p, "float*": C.c_void_p,
             "uint8_t*": C.c_void_p, "const int32_t*": C.c_void_p}
    for name in ENTRIES:
        m = re.search(r"\b(int|long long)\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, f"{name} is not declared in include/neube_hip.h"
        params = [re.sub(r"\s*\b\w+$", "", p.strip()).replace(" *", "*") for p in m.group(2).split(",")]
        res, args = _lib.PROTOTYPES[name]
        assert res is {"int": C.c_int, "long long": C.c_longlong}[m.group(1)] and args == [ctype[p] for p in params], (name, params)
        assert hasattr(library, name)
    m = re.search(r"#define\s+NB_SEG_PITCH\s+(\d+)", text)
    assert m and int(m.group(1)) == _lib.NB_SEG_PITCH == painting.SEG_PITCH == 8
    common = open(os.path.join(REPO, "brushstroke_engine_amd", "csrc", "nb_common.h")).read()
    assert int(re.search(r"#define NB_ABI_VERSION (\d+)", common).group(1)) == _lib.ABI_VERSION >= 19
    assert "nb_strokes.hip" in build.SOURCES and "-fno-slp-vectorize" in build.FILE_FLAGS["nb_strokes.hip"]
    # the CPU stand-ins inherit the numpy restatement; TileOps overrides it with the kernels
    assert hasattr(painting.TileOpsBase, "raster_strokes") and painting.TileOps.raster_strokes is not painting.TileOpsBase.raster_strokes


# ---------------------------------------------------------------------------------------------------------------------
# paint_strokes on the oracle-backed ops, and the command line
# ---------------------------------------------------------------------------------------------------------------------
def test_base_raster_strokes_is_the_numpy_restatement():
    strokes, ops = sr.e2e_strokes(), painting.TileOpsBase()
    h, w = sr.E2E_SIZE[0] + 20, sr.E2E_SIZE[1] + 20
    want = painting.raster_strokes_numpy(strokes, (h, w), (10, 10), subdiv=8)
    got = ops.raster_strokes(strokes, (h, w), (10, 10))
    assert got.dtype == torch.uint8 and np.array_equal(got.numpy(), want) and 0 < (want == 0).mean() < 0.2
    # ``out`` given: darkened in place, every other byte as it was
    base = np.random.RandomState(1).randint(1, 256, (h, w)).astype(np.uint8)
    out = torch.from_numpy(base.copy())
    assert ops.raster_strokes(strokes, offset=(10, 10), out=out) is out
    assert np.array_equal(out.numpy(), np.where(want == 0, 0, base))


def test_paint_strokes_on_the_oracle_ops_equals_the_host_route():
    """``paint_strokes`` takes its one route -- raster, clear the padding, ``_paint_padded`` -- on the oracle-backed ops and returns the
    bytes of ``paint_image(raster_strokes_numpy(strokes, size)[..., None], ...)``, in every case of ``cr.ROUTE_CASES`` (1-2 s each)."""
    strokes = cr.session_strokes()[0]
    for case in cr.ROUTE_CASES:
        print("case (level, mode, on_white):", case)
        cr.check_same_as_host_route(lambda helper, opts, **kw: helper.paint_strokes(strokes, cr.ROUTE_SIZE, opts, **kw), case)


def test_paint_strokes_refuses_an_empty_drawing():
    with pytest.raises(ValueError):
        cr.route_helper(0).paint_strokes(cr.session_strokes()[0], (0, 120), painting.GanBrushOptions())


def test_parser_takes_strokes_or_a_drawing(capsys):
    ap = paint_image_main.build_parser()
    base = ["--gan_checkpoint", "e.npz", "--output_file_prefix", "out/x", "--style_id", "594"]
    a = ap.parse_args(base + ["--strokes", "s.json", "--canvas_size", "514,800"])
    assert a.strokes == "s.json" and a.geom_image is None and paint_image_main.parse_canvas_size(a.canvas_size) == (514, 800)
    for argv in (base, base + ["--strokes", "s.json", "--geom_image", "d.png", "--canvas_size", "5,5"]):     # neither, both
        with pytest.raises(SystemExit):
            ap.parse_args(argv)
    # today's argument lists parse as before
    b = ap.parse_args(base + ["--geom_image", "d.png", "--feature_blending_level", "2", "--on_white", "--stitching_mode", "stroke",
                              "--library", "594,12", "--no_uvs_mapping", "--host_prepare", "--gpus", "2", "--conv_mode", "h3"])
    assert (b.geom_image, b.strokes, b.canvas_size, b.feature_blending_level, b.on_white, b.host_prepare, b.gpus) == \
        ("d.png", None, None, 2, True, True, 2)
    # --strokes without a size (and a size without strokes, and a malformed size) end in a parser error before anything is loaded
    for argv in (base + ["--strokes", "s.json"], base + ["--geom_image", "d.png", "--canvas_size", "5,5"],
                 base + ["--strokes", "s.json", "--canvas_size", "5x5"], base + ["--strokes", "s.json", "--canvas_size", "0,5"]):
        with pytest.raises(SystemExit):
            paint_image_main.main(argv)
    capsys.readouterr()
