"""What the CPU and the GPU tests of the compositing kernels and the paint session share (tests/test_compose_cpu.py,
tests/test_hip_compose.py): the scenes, the contract of the view as a loop, and the assertions on a session -- and the drawing,
cases and once-computed ``paint_image`` results that hold ``paint_strokes`` and ``paint_drawing`` to the host route on the CPU."""
import functools

import numpy as np
import torch

from brushstroke_engine_amd import painting

OPACITIES = (255, 128, 1, 0)
# (source colour, destination colour): extremes both ways, and two mixed pairs
COLOUR_PAIRS = (((255, 255, 255), (0, 0, 0)), ((0, 0, 0), (255, 255, 255)), ((200, 37, 1), (3, 254, 128)), ((127, 128, 255), (128, 127, 254)))


def alpha_square(cs, cd):
    """One 256 x 256 tile whose alpha is the row, and a canvas whose alpha is the column."""
    tile = np.empty((1, 256, 256, 4), np.uint8)
    tile[0, :, :, :3] = cs
    tile[0, :, :, 3] = np.arange(256, dtype=np.uint8)[:, None]
    canvas = np.empty((256, 256, 4), np.uint8)
    canvas[:, :, :3] = cd
    canvas[:, :, 3] = np.arange(256, dtype=np.uint8)[None, :]
    return tile, canvas


def over_scene(h=117, w=131, seed=5):
    """Seven tiles of r = 40 with crop 3 at stride 28 (neighbouring interiors overlap by 6 pixels) on an h x w canvas: two origins are
    negative, the last tile hangs over the far edge.  -> (tiles, dst_yx, crop, canvas, a pixel box smaller than the tiles' extent)."""
    rs = np.random.RandomState(seed)
    tiles = rs.randint(0, 256, (7, 40, 40, 4)).astype(np.uint8)
    tiles[rs.rand(7, 40, 40) < 0.25, 3] = 0
    tiles[rs.rand(7, 40, 40) < 0.25, 3] = 255
    yx = np.array([[-10, -6], [18, -12], [18, 22], [46, 50], [46, 78], [74, 78], [90, 106]], np.int32)
    canvas = rs.randint(0, 256, (h, w, 4)).astype(np.uint8)
    canvas[rs.rand(h, w) < 0.3, 3] = 0
    return tiles, yx, 3, canvas, (22, 10, 101, 120)


def view_loop(canvas, y0, x0, h, w, k, on_white):
    """The contract of nb_canvas_view_u8 block by block in Python integers."""
    oh, ow = -(-h // k), -(-w // k)
    out = np.zeros((oh, ow, 3 if on_white else 4), np.uint8)
    for oy in range(oh):
        for ox in range(ow):
            blk = canvas[y0 + oy * k:y0 + min(h, oy * k + k), x0 + ox * k:x0 + min(w, ox * k + k)].reshape(-1, 4).tolist()
            n = len(blk)
            sa = sum(p[3] for p in blk)
            sc = [sum(p[c] * p[3] for p in blk) for c in range(3)]
            if on_white:
                out[oy, ox] = [(s + 255 * (255 * n - sa) + (255 * n) // 2) // (255 * n) for s in sc]
            else:
                out[oy, ox] = [(s + sa // 2) // sa if sa > 0 else 0 for s in sc] + [(sa + n // 2) // n]
    return out


def view_canvas(ch=140, cw=150, seed=11):
    """Random RGBA with runs of transparent and of opaque pixels; one 16-aligned block of the (5, 9) window all transparent."""
    rs = np.random.RandomState(seed)
    canvas = rs.randint(0, 256, (ch, cw, 4)).astype(np.uint8)
    canvas[rs.rand(ch, cw) < 0.3, 3] = 0
    canvas[rs.rand(ch, cw) < 0.2, 3] = 255
    canvas[5 + 32:5 + 48, 9 + 48:9 + 64, 3] = 0
    return canvas


VIEW_WINDOW = (5, 9, 117, 131)
SIZE = (150, 150)


def session_strokes():
    """Two short strokes of a 150 x 150 drawing that reach all four tiles of its grid (R = 128, margin 10: tiles at 0 and 88)."""
    first = painting.StrokeList().add_polyline([[70.5, 60.0], [112.0, 84.5]], 5.0).add_spline([[60.0, 100.0], [75.5, 112.0], [96.0, 108.5]], [3.0, 4.5, 3.5])
    second = painting.StrokeList().add_polyline([[90.0, 50.5], [78.0, 118.0]], 6.0)          # crosses both strokes of the first layer
    outside = painting.StrokeList().add_polyline([[200.0, 170.0], [260.0, 180.0]], 5.0).add_polyline([[-40.0, 20.0], [-12.0, 30.0]], 4.0)
    return first, second, outside


def session_brushes(z_dim):
    a = painting.GanBrushOptions()
    a.set_style(torch.from_numpy(np.random.RandomState(594).randn(1, z_dim)), 594)
    b = painting.GanBrushOptions(primary_color=np.array([200, 30, 40], np.uint8), secondary_color=np.array([20, 60, 220], np.uint8))
    b.set_style(torch.from_numpy(np.random.RandomState(12).randn(1, z_dim)), 12)
    return a, b


def check_session(ops, level, m, to_host):
    """What both the CPU and the GPU test of the session assert; returns the session (two layers minus one undo = one layer)."""
    first, second, outside = session_strokes()
    brush_a, brush_b = session_brushes(ops.cfg.z_dim)

    def reference(strokes, opts):
        helper = painting.PaintingHelper(ops, batch=4)
        helper.set_feature_blending(level)
        image, full, crops, _ = helper.paint_strokes(strokes, SIZE, opts, crop_margin=m, stitching_mode="stroke", on_white=True,
                                                     return_full=True)
        return image, full, crops
    helper = painting.PaintingHelper(ops, batch=4)
    helper.set_feature_blending(level)
    session = painting.PaintSession(helper, SIZE, crop_margin=m)
    assert tuple(session.canvas.shape) == (304, 304, 4) and not to_host(session.canvas).any()
    box = session.add(first, brush_a)
    image1, full1, crops1 = reference(first, brush_a)
    assert len(crops1) == 4 and full1[..., 3].max() > 0
    one = to_host(session.canvas).copy()
    assert np.array_equal(session.image(on_white=True), image1)
    assert np.array_equal(one[..., 3], full1[..., 3]) and np.array_equal(one[one[..., 3] > 0], full1[full1[..., 3] > 0])
    assert np.array_equal(session.image(), one[m:m + 150, m:m + 150])
    changed = np.argwhere(one[m:m + 150, m:m + 150].any(axis=2))
    assert box[0] <= changed[:, 0].min() and box[1] <= changed[:, 1].min() and box[2] > changed[:, 0].max() and box[3] > changed[:, 1].max()
    # a second brush over the first
    box2 = session.add(second, brush_b)
    _, full2, crops2 = reference(second, brush_b)
    assert len(crops2) >= 2 and box2 != painting.EMPTY_BOX
    two = to_host(session.canvas).copy()
    want = painting.over_tiles_numpy(full1.copy(), full2[None], [[0, 0]], 0)
    assert np.array_equal(two, want) and not np.array_equal(two, one)
    assert ((full1[..., 3] > 0) & (full2[..., 3] > 0)).any()                           # the layers do overlap
    assert np.array_equal(session.view(k=4, on_white=True), painting.canvas_view_numpy(two, m, m, 150, 150, 4, True))
    assert np.array_equal(session.view(box=(10, 20, 97, 131), k=3), painting.canvas_view_numpy(two, m + 10, m + 20, 87, 111, 3, False))
    # strokes wholly outside the drawing: nothing happens, and nothing is remembered for undo
    assert session.add(outside, brush_b) == painting.EMPTY_BOX and session.add(painting.StrokeList(), brush_b) == painting.EMPTY_BOX
    assert np.array_equal(to_host(session.canvas), two)
    assert session.undo() == box2
    assert np.array_equal(to_host(session.canvas), one)
    return session


# ---------------------------------------------------------------------------------------------------------------------
# one route whatever the ops: paint_strokes / paint_drawing on the oracle-backed ops against the host route paint_image
# (tests/test_stroke_refs_cpu.py, tests/test_geomprep_cpu.py)
# ---------------------------------------------------------------------------------------------------------------------
# 150 x 170 at R = 128, crop margin 10: tiles at stride 88 in 2 rows x 3 columns, neighbours overlapping by 40 px, and a third column
# without a stroke pixel, which "stroke" mode drops -- the smallest drawing with all of that.
ROUTE_SIZE = (150, 170)
ROUTE_CASES = [(level, mode, on_white) for level in (0, 2) for mode in ("stroke", "all") for on_white in (False, True)]
ROUTE_FULL_CASE = (2, "stroke", True)            # the one case that also compares canvas, crops and padded geometry


@functools.lru_cache(maxsize=None)
def route_ops():
    """(ops, crop margin): ``OracleTileOps`` on the weights of ``engine_r128.npz``, as tests/test_compose_cpu.py sets it up."""
    from conftest import load_golden
    from brushstroke_engine_amd import config as cfgmod, encoder as encmod, weights as wmod
    from oracle_tile_ops import OracleTileOps
    g = load_golden("engine_r128.npz")
    cfg = cfgmod.style1_config(int(g["resolution"]))
    ops = OracleTileOps(cfg, wmod.random_state_dict(cfg, seed=int(g["weights_seed"])), encmod.random_encoder_state_dict(int(g["encoder_seed"])))
    return ops, int(g["crop_margin"])


def route_helper(level):
    helper = painting.PaintingHelper(route_ops()[0], batch=4)
    helper.set_feature_blending(level)
    return helper


@functools.lru_cache(maxsize=None)
def route_geometry():
    """[150, 170, 1] uint8, read-only: the first session strokes rasterised on the host."""
    geom = painting.raster_strokes_numpy(session_strokes()[0], ROUTE_SIZE)[..., None]
    geom.flags.writeable = False
    return geom


@functools.lru_cache(maxsize=None)
def host_route(level, mode, on_white):
    """(image, canvas, crops, padded geometry) of ``paint_image`` on ``route_geometry()``, computed once per case, read-only."""
    ops, m = route_ops()
    with torch.no_grad():
        out = route_helper(level).paint_image(route_geometry(), session_brushes(ops.cfg.z_dim)[0], crop_margin=m, stitching_mode=mode,
                                              on_white=on_white, return_full=True)
    for a in (out[0], out[1], out[3]):
        a.flags.writeable = False
    return out


def check_same_as_host_route(paint, case):
    """``paint(helper, opts, crop_margin=, stitching_mode=, on_white=, return_full=)`` -- paint_strokes or paint_drawing on the drawing of
    ``route_geometry()`` -- returns the bytes of the host route, and those are a painting, not a blank."""
    level, mode, on_white = case
    ops, m = route_ops()
    image, canvas, crops, padded = host_route(*case)
    assert (route_geometry() == 0).sum() > 500 and (padded == 0).sum() == (route_geometry() == 0).sum()
    assert image.shape == ROUTE_SIZE + ((3,) if on_white else (4,)) and len(np.unique(image.reshape(-1, image.shape[2]), axis=0)) > 10
    assert len(crops) == (4 if mode == "stroke" else 6)
    full = case == ROUTE_FULL_CASE
    with torch.no_grad():
        got = paint(route_helper(level), session_brushes(ops.cfg.z_dim)[0], crop_margin=m, stitching_mode=mode, on_white=on_white,
                    return_full=full)
    if not full:
        assert got.dtype == np.uint8 and np.array_equal(got, image)
        return
    assert np.array_equal(got[0], image) and np.array_equal(got[1], canvas) and canvas.any()
    assert [tuple(c) for c in got[2]] == [tuple(c) for c in crops] and got[3].dtype == np.uint8 and np.array_equal(got[3], padded)


def good_script():
    first, second, _ = session_strokes()
    return {"size": [150, 150], "crop_margin": 10, "feature_blending_level": 2,
            "layers": [{"strokes": first.items, "library": "594,12", "style_id": "594"},
                       {"strokes": second.items, "library": "594,12", "style_id": "12", "colors": [[200, 30, 40], None, [20, 60, 220]],
                        "mode": "erase", "opacity": 128}]}
