"""CPU checks of the staged C generator entry and the canvas helpers of a C host (no GPU): nb_canvas_build_cells against
painting.build_cells, the argument errors of nb_generator_forward_staged / nb_generator_describe_staged that need no device, and
examples/capi/paint_blended.c building against the library."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from brushstroke_engine_amd import _lib, build, painting
from conftest import load_golden

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def library():
    build.build()
    return _lib.lib()


def c_build_cells(library, rects, h, w):
    r = np.ascontiguousarray(np.asarray(rects, np.int32).reshape(-1, 4))
    t = r.shape[0]
    ptr = r.ctypes.data if t else None
    count = library.nb_canvas_cells_count(ptr, t, h, w)
    assert count >= 1, library.nb_last_error()
    ncells = -(-h // painting.CELL_H) * -(-w // painting.CELL_W)
    off = np.full(ncells + 1, -7, np.int32)
    items = np.full(count + 1, -7, np.int32)             # (one guard entry behind the list)
    assert library.nb_canvas_build_cells(ptr, t, h, w, off.ctypes.data, items.ctypes.data) == _lib.NB_OK, library.nb_last_error()
    assert items[count] == -7
    return off, items[:count], count


def engine_rects(level):
    """The rectangles PaintingHelper builds cells from for engine_r128.npz (9 tiles, R = 128, crop margin 10): the pasted interiors
    (level 0) or the tile areas on the feature canvas (level 2: floored to the blending grid, painting.py render_tiles / _schedule)."""
    g = load_golden("engine_r128.npz")
    R, m = 128, int(g["crop_margin"])
    geom = g["geom"][..., None] if g["geom"].ndim == 2 else g["geom"]
    crops, padded = painting.generate_stitching_crops(painting.pad_geo(geom, m), R, "all", 2 * m)
    yx = np.asarray([c[:2] for c in crops], np.int64)
    H, W = padded.shape[:2]
    if level == 0:
        return np.concatenate([yx + m, yx + R - m], axis=1), H, W
    df = 2 ** (level - 1)
    fl = (yx // df) * df
    return np.concatenate([fl // df, fl // df + R // df], axis=1), -(-H // df), -(-W // df)


def random_rects(n, h, w, seed):
    rs = np.random.RandomState(seed)
    y0, x0 = rs.randint(-40, h + 20, n), rs.randint(-90, w + 50, n)
    return np.stack([y0, x0, y0 + rs.randint(-3, 200, n), x0 + rs.randint(-3, 300, n)], 1)      # (some empty, some inverted)


CELL_CASES = {
    "empty": (np.zeros((0, 4), np.int64), 37, 130),
    "outside": (np.array([[-50, -70, -1, -2], [-5, -5, 3, 70], [30, 100, 90, 400], [40, 130, 50, 140], [37, 0, 80, 10], [10, 20, 10, 90],
                          [0, 0, 0, 0], [36, 129, 37, 130]]), 37, 130),
    "all": (np.array([[0, 0, 517, 1030]]), 517, 1030),
    "random": (random_rects(2000, 517, 1030, 3), 517, 1030),            # a 1030-wide grid of 517 rows: ragged last cells both ways
    "engine_level0": engine_rects(0),
    "engine_level2": engine_rects(2),
}


@pytest.mark.parametrize("case", list(CELL_CASES))
def test_build_cells_equals_python(library, case):
    rects, h, w = CELL_CASES[case]
    want_off, want_items = painting.build_cells(rects, h, w)
    off, items, count = c_build_cells(library, rects, h, w)
    assert count == len(want_items)
    np.testing.assert_array_equal(off, want_off)
    np.testing.assert_array_equal(items, want_items)
    if case.startswith("engine") or case in ("all", "random"):
        assert off[-1] == count and count > 1              # (the case does fill cells)


def test_build_cells_bad_arguments(library):
    r = np.zeros((1, 4), np.int32)
    assert library.nb_canvas_cells_count(None, 1, 8, 8) == _lib.NB_EINVAL and b"null rectangles" in library.nb_last_error()
    assert library.nb_canvas_cells_count(r.ctypes.data, 1, 0, 8) == _lib.NB_EINVAL and b"bad grid size" in library.nb_last_error()
    assert library.nb_canvas_build_cells(r.ctypes.data, 1, 8, 8, None, None) == _lib.NB_EINVAL and b"null output" in library.nb_last_error()


def test_staged_argument_errors_without_gpu(library):
    ins, outs = _lib.NbGeneratorInputs(), _lib.NbGeneratorOutputs()
    fake = ctypes.c_void_p(16)                             # (never dereferenced: every case fails before the handle is read)
    buf = ctypes.create_string_buffer(64)

    def forward(gen, stage):
        return library.nb_generator_forward_staged(gen, ctypes.byref(ins), None, None if stage is None else ctypes.byref(stage),
                                                   ctypes.byref(outs), 1, None)

    cases = [("null handle", None, _lib.NbGeneratorStage(64, 0, 16, None), b"null pointer"),
             ("null stage", fake, None, b"null stage"),
             ("both set", fake, _lib.NbGeneratorStage(64, 32, 16, 16), b"exactly one of stop_res / resume_res"),
             ("both zero", fake, _lib.NbGeneratorStage(0, 0, 16, 16), b"exactly one of stop_res / resume_res"),
             ("no block: 48", fake, _lib.NbGeneratorStage(48, 0, 16, None), b"48 is not a block resolution"),
             ("no block: 2", fake, _lib.NbGeneratorStage(0, 2, None, 16), b"2 is not a block resolution"),
             ("no block: -64", fake, _lib.NbGeneratorStage(-64, 0, 16, None), b"-64 is not a block resolution")]
    for what, gen, stage, msg in cases:
        assert forward(gen, stage) == _lib.NB_EINVAL, what
        assert msg in library.nb_last_error(), (what, library.nb_last_error())
    assert library.nb_generator_forward_staged(fake, None, None, ctypes.byref(_lib.NbGeneratorStage(64, 0, 16, None)), None, 1, None) == _lib.NB_EINVAL
    assert b"null pointer" in library.nb_last_error()
    for stop, resume, msg in [(64, 32, b"exactly one"), (0, 0, b"exactly one"), (24, 0, b"24 is not a block resolution")]:
        assert library.nb_generator_describe_staged(fake, 1, stop, resume, buf, 64) == _lib.NB_EINVAL
        assert msg in library.nb_last_error()
    assert library.nb_generator_describe_staged(None, 1, 64, 0, buf, 64) == _lib.NB_EINVAL and b"bad arguments" in library.nb_last_error()
    assert ctypes.sizeof(_lib.NbGeneratorStage) == 24      # two int32, two pointers
    # the whole text of one failing call per entry
    assert forward(None, _lib.NbGeneratorStage(64, 0, 16, None)) == _lib.NB_EINVAL
    assert library.nb_last_error() == b"generator_forward_staged: null pointer"
    assert library.nb_generator_describe_staged(None, 1, 64, 0, buf, 64) == _lib.NB_EINVAL
    assert library.nb_last_error() == b"generator_describe_staged: bad arguments"
    assert library.nb_generator_describe_staged(fake, 1, 24, 0, buf, 64) == _lib.NB_EINVAL
    assert library.nb_last_error() == b"generator_describe_staged: 24 is not a block resolution (a power of two in [4, R])"


def test_dirty_area_alpha_argument_errors_without_gpu(library):
    for width, margin, crop, msg in [(64, 0, 5, b"bad sizes"), (64, -1, 0, b"bad sizes"), (64, 22, 10, b"leave no interior"),
                                     (16, 8, 0, b"leave no interior")]:
        assert library.nb_dirty_area_alpha_f32(16, width, margin, crop, None) == _lib.NB_EINVAL
        assert msg in library.nb_last_error()
    assert library.nb_dirty_area_alpha_f32(None, 64, 8, 5, None) == _lib.NB_EINVAL and b"null pointer" in library.nb_last_error()


def test_paint_blended_example_builds(library, tmp_path):
    cmd = ["cc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__",
           os.path.join(REPO, "examples", "capi", "paint_blended.c"), "-o", str(tmp_path / "paint_blended"), "-L/opt/rocm/lib", "-lamdhip64",
           "-L" + os.path.dirname(_lib.LIB_PATH), "-lneube_hip"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert os.path.exists(tmp_path / "paint_blended")
