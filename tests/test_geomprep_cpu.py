"""Drawing preparation, the parts that need no GPU: the host-only tile grid ``nb_stitching_grid`` against
``painting.generate_stitching_crops``, argument checks of the device entries (they validate before any launch), the
header / binding agreement on the four entries of ``csrc/nb_geomprep.hip``, the host restatements ``TileOpsBase`` carries for them,
and ``paint_drawing`` on the oracle-backed ops against the host route ``paint_image``."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import compose_refs as cr
from brushstroke_engine_amd import _lib, build, painting

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("nb_geom_prepare_u8", "nb_tile_stroke_counts_u8", "nb_composite_on_white_u8", "nb_stitching_grid")


@pytest.fixture(scope="module")
def library():
    build.build()
    return _lib.lib()


def _grid(library, h, w, r, overlap):
    v = [C.c_int(-7) for _ in range(5)]
    rc = library.nb_stitching_grid(h, w, r, overlap, *[C.byref(x) for x in v])
    return rc, tuple(x.value for x in v)


# strides: 128 - 40 = 88, 256 - 40 = 216, 32 - 2 = 30, 16 (no overlap), 1 (the smallest legal one)
@pytest.mark.parametrize("r,overlap", [(128, 20), (256, 20), (32, 1), (16, 0), (9, 4)])
def test_stitching_grid_matches_generate_stitching_crops(library, r, overlap):
    stride = r - 2 * overlap
    sizes = sorted({1, 2, stride - 1, stride, stride + 1, 2 * stride - 1, 2 * stride, 2 * stride + 1, 3 * stride, 5 * stride + 3, 37})
    sizes = [s for s in sizes if s >= 1]
    for h in sizes:
        for w in sizes:
            crops, padded = painting.generate_stitching_crops(np.zeros((h, w, 1), np.uint8), r, "all", overlap)
            rc, (nrows, ncols, st, ph, pw) = _grid(library, h, w, r, overlap)
            assert rc == 0
            assert st == stride and (ph, pw) == padded.shape[:2], (h, w)
            assert [(row * st, col * st, r, r) for row in range(nrows) for col in range(ncols)] == crops, (h, w)
            assert painting.stitching_grid(h, w, r, overlap) == (nrows, ncols, st, ph, pw)


def test_stitching_grid_rejects_bad_arguments(library):
    for r, overlap in [(128, 64), (128, 65), (10, 5), (1, 1)]:             # patch_width - 2 * overlap_margin <= 0
        rc, vals = _grid(library, 100, 100, r, overlap)
        assert rc == _lib.NB_EINVAL and vals == (-7,) * 5
        assert b"overlap margin" in library.nb_last_error()
    one = C.c_int()
    assert library.nb_stitching_grid(10, 10, 128, 20, C.byref(one), C.byref(one), C.byref(one), C.byref(one), None) == _lib.NB_EINVAL
    with pytest.raises(_lib.NeubeHipError):
        painting.stitching_grid(10, 10, 40, 20)


def test_device_entries_validate_on_the_host(library):
    """Bad arguments are refused before any launch (no GPU needed); the pointers are never dereferenced on the host."""
    p = 0x1000
    ok = dict(img=p, h=8, w=8, ch=3, out=p, oh=8, ow=8, oy=0, ox=0, ws=p)

    def prep(**kw):
        a = dict(ok, **kw)
        return library.nb_geom_prepare_u8(a["img"], a["h"], a["w"], a["ch"], a["out"], a["oh"], a["ow"], a["oy"], a["ox"], a["ws"], None)
    for bad in (dict(ch=2), dict(ch=0), dict(ch=5), dict(img=None), dict(out=None), dict(ws=None), dict(oy=1), dict(ox=1),
                dict(oh=7), dict(ow=7), dict(oy=-1, oh=16), dict(h=0), dict(w=0)):
        assert prep(**bad) == _lib.NB_EINVAL, bad
    assert library.nb_tile_stroke_counts_u8(None, 8, 8, 4, 4, 1, 1, p, None) == _lib.NB_EINVAL
    assert library.nb_tile_stroke_counts_u8(p, 8, 8, 4, 0, 1, 1, p, None) == _lib.NB_EINVAL
    assert library.nb_composite_on_white_u8(p, 8, 8, 4, 4, 5, 4, p, None) == _lib.NB_EINVAL       # window leaves the canvas
    assert library.nb_composite_on_white_u8(p, 8, 8, 0, 0, 8, 8, None, None) == _lib.NB_EINVAL


def test_header_and_binding_agree_on_the_entries(library):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "neube_hip.h")).read(), flags=re.S)
    ctype = {"int": C.c_int, "void*": C.c_void_p, "const uint8_t*": C.c_void_p, "uint8_t*": C.c_void_p, "int32_t*": C.c_void_p,
             "int*": C.POINTER(C.c_int)}
    for name in ENTRIES:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, f"{name} is not declared in include/neube_hip.h"
        params = [re.sub(r"\s*\b\w+$", "", p.strip()).replace(" *", "*") for p in m.group(1).split(",")]
        res, args = _lib.PROTOTYPES[name]
        assert res is C.c_int and args == [ctype[p] for p in params], (name, params)
        assert hasattr(library, name)
    m = re.search(r"#define\s+NB_GEOM_PREP_WS_BYTES\s+(\d+)", text)
    assert m and int(m.group(1)) == _lib.NB_GEOM_PREP_WS_BYTES == (4 + 256) * 4
    common = open(os.path.join(REPO, "brushstroke_engine_amd", "csrc", "nb_common.h")).read()
    assert int(re.search(r"#define NB_ABI_VERSION (\d+)", common).group(1)) == _lib.ABI_VERSION >= 16
    assert "nb_geomprep.hip" in build.SOURCES


def test_the_base_ops_restate_the_preparation_and_tile_ops_overrides_it():
    """The CPU stand-ins inherit the host restatements; TileOps overrides them with the kernels."""
    for name in ("prepare_geometry", "stroke_counts", "composite_on_white", "raster_strokes"):
        assert hasattr(painting.TileOpsBase, name) and getattr(painting.TileOps, name) is not getattr(painting.TileOpsBase, name)
    ops = painting.TileOpsBase()
    rs = np.random.RandomState(2)
    geom = np.where(rs.rand(45, 70) < 0.3, 0, 255).astype(np.uint8)
    counts = ops.stroke_counts(torch.from_numpy(geom), 32, 20, 2, 3)
    padded = np.full((20 + 32, 40 + 32 + 10), 255, np.uint8)
    padded[:45, :70] = geom
    want = [[int((padded[y:y + 32, x:x + 32] == 0).sum()) for x in (0, 20, 40)] for y in (0, 20)]
    assert counts.dtype == torch.int32 and counts.tolist() == want and min(map(min, want)) > 10
    assert painting.tiles_with_strokes(np.array([[11, 10, 0], [0, 12, 300]]), 7).tolist() == [[0, 0], [7, 7], [7, 14]]
    img = rs.randint(0, 256, (21, 33, 4)).astype(np.uint8)
    out = ops.prepare_geometry(img, (40, 50), (3, 5))
    want = np.full((40, 50), 255, np.uint8)
    want[3:24, 5:38] = painting.prepare_geometry_image(img)[..., 0]
    assert out.dtype == torch.uint8 and np.array_equal(out.numpy(), want) and (want[3:24, 5:38] == 0).any()
    canvas = torch.from_numpy(rs.randint(0, 256, (30, 40, 4)).astype(np.uint8))
    a = canvas[2:22, 3:33, 3:].numpy().astype(np.float32) / np.float32(255)
    white = (canvas[2:22, 3:33, :3].numpy().astype(np.float32) * a + 255 * (1 - a)).clip(0, 255).astype(np.uint8)
    assert np.array_equal(ops.composite_on_white(canvas, 2, 3, 20, 30).numpy(), white)


def test_paint_drawing_on_the_oracle_ops_equals_the_host_route():
    """``paint_drawing`` takes its one route -- ``_paint_padded`` -- on the oracle-backed ops and returns the bytes of
    ``paint_image(prepare_geometry_image(rgba), ...)``, in every case of ``cr.ROUTE_CASES`` (1-2 s each)."""
    geom = cr.route_geometry()
    rgba = np.zeros(cr.ROUTE_SIZE + (4,), np.uint8)
    rgba[geom[..., 0] == 0] = (0, 0, 0, 255)                          # the strokes, opaque black on a transparent sheet
    assert np.array_equal(painting.prepare_geometry_image(rgba), geom)
    for case in cr.ROUTE_CASES:
        print("case (level, mode, on_white):", case)
        cr.check_same_as_host_route(lambda helper, opts, **kw: helper.paint_drawing(rgba, opts, **kw), case)


def test_paint_drawing_refuses_other_than_uint8_drawings():
    helper = cr.route_helper(0)
    for bad in (np.zeros((40, 50, 4), np.float32), np.zeros((40, 50, 2), np.uint8), np.zeros((40,), np.uint8)):
        with pytest.raises(ValueError):
            helper.paint_drawing(bad, painting.GanBrushOptions())
