"""Drawing preparation, the parts that need no GPU: the host-only tile grid ``nb_stitching_grid`` against
``painting.generate_stitching_crops``, argument checks of the device entries (they validate before any launch), and the
header / binding agreement on the four entries of ``csrc/nb_geomprep.hip``."""
import ctypes as C
import os
import re

import numpy as np
import pytest

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


class _NoPrepOps(painting.TileOpsBase):
    """What the CPU stand-ins of TileOps look like to paint_drawing: no preparation kernels."""
    patch_width = 128


def test_paint_drawing_falls_back_to_the_numpy_helpers(monkeypatch):
    helper = painting.PaintingHelper(_NoPrepOps())
    rgba = np.zeros((40, 50, 4), np.uint8)
    rgba[8:12, :, 3] = 255
    seen = {}

    def fake_paint_image(geom, opts, **kw):
        seen.update(geom=geom, opts=opts, **kw)
        return "painted"
    monkeypatch.setattr(helper, "paint_image", fake_paint_image)
    assert helper.paint_drawing(rgba, "opts", crop_margin=7, stitching_mode="stroke", on_white=True) == "painted"
    assert np.array_equal(seen["geom"], painting.prepare_geometry_image(rgba))
    assert (seen["opts"], seen["crop_margin"], seen["stitching_mode"], seen["on_white"], seen["return_full"]) == ("opts", 7, "stroke", True, False)
