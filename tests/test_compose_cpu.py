"""CPU checks of the paint session: the numpy restatements of the two compositing contracts (include/neube_hip.h,
csrc/nb_compose.hip) against their definitions, the exported entries, ``painting.PaintSession`` on the oracle-backed ops, and the
script parser of ``paint_session_main``."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from conftest import load_golden
from brushstroke_engine_amd import _lib, build, config as cfgmod, encoder as encmod, paint_session_main, painting, weights as wmod
import compose_refs as cr
from oracle_tile_ops import OracleTileOps

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------------
# the restatements against their definitions
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opacity", cr.OPACITIES)
def test_over_restatement_against_its_definition(opacity):
    a_s, a_d = np.meshgrid(np.arange(256, dtype=np.int64), np.arange(256, dtype=np.int64), indexing="ij")
    ae = (a_s * opacity + 127) // 255
    t = a_d * (255 - ae)
    den = ae * 255 + t
    largest = 0
    for cs, cd in cr.COLOUR_PAIRS:
        tile, canvas = cr.alpha_square(cs, cd)
        got = painting.over_tiles_numpy(canvas.copy(), tile, [[0, 0]], 0, 0, opacity).astype(np.int64)
        assert np.array_equal(got[..., 3], (den + 127) // 255)
        for c in range(3):
            num = cs[c] * ae * 255 + cd[c] * t
            largest = max(largest, int((num + den // 2).max()))
            # the integer nearest to num / den, ties up: floor((2 num + den) / (2 den))
            want = np.where(den > 0, (2 * num + den) // np.maximum(2 * den, 1), 0)
            assert np.array_equal(got[..., c], want), (cs, cd, c)
        # a transparent destination yields (cs, ae); a transparent source leaves alpha (and a visible colour) as they were
        assert np.array_equal(got[:, 0, 3], ae[:, 0]) and (got[ae[:, 0] > 0, 0, :3] == cs).all()
        src0 = ae == 0
        assert np.array_equal(got[..., 3][src0], a_d[src0]) and (got[src0 & (a_d > 0)][:, :3] == cd).all()
        assert (got[(ae == 0) & (a_d == 0)] == 0).all()
        # erase: destination-out by the stroke's alpha, colour untouched
        out = painting.over_tiles_numpy(canvas.copy(), tile, [[0, 0]], 0, 1, opacity).astype(np.int64)
        assert np.array_equal(out[..., 3], (a_d * (255 - ae) + 127) // 255) and (out[..., :3] == cd).all()
    assert largest <= 16_613_887 < 2 ** 24
    if opacity == 255:
        assert largest == 16_613_887


def test_over_restatement_selects_tiles_like_the_paste():
    """The last interior that covers a pixel is its source; pixels without one, and pixels outside the cell box, keep their bytes."""
    rs = np.random.RandomState(3)
    tiles = rs.randint(0, 256, (3, 40, 40, 4)).astype(np.uint8)
    yx = np.array([[-5, -7], [10, 20], [30, 100]])
    canvas = rs.randint(0, 256, (60, 131, 4)).astype(np.uint8)
    full = painting.over_tiles_numpy(canvas.copy(), tiles, yx, 3)
    want = canvas.copy()
    last = np.full((60, 131), -1)
    for i, (y, x) in enumerate(yx.tolist()):
        last[max(0, y + 3):min(60, y + 37), max(0, x + 3):min(131, x + 37)] = i
    for i in range(3):                                            # ONE source per pixel: the last tile's, over the canvas as it was
        one = painting.over_tiles_numpy(canvas.copy(), tiles[i:i + 1], yx[i:i + 1], 3)
        want[last == i] = one[last == i]
    assert np.array_equal(full, want) and np.array_equal(full[last < 0], canvas[last < 0]) and (last >= 0).any() and (last < 0).any()
    boxed = painting.over_tiles_numpy(canvas.copy(), tiles, yx, 3, cells=painting.cell_box((8, 0, 20, 64), 60, 131))
    inside = np.zeros((60, 131), bool)
    inside[8:20, 0:64] = True
    assert np.array_equal(boxed[inside], full[inside]) and np.array_equal(boxed[~inside], canvas[~inside])
    assert painting.cell_box((8, 70, 21, 130), 60, 131) == (1, 2, 2, 4) and painting.cell_box((70, 0, 80, 5), 60, 131) is None
    with pytest.raises(ValueError):
        painting.over_tiles_numpy(canvas.copy(), tiles, yx, 3, mode=2)
    with pytest.raises(ValueError):
        painting.over_tiles_numpy(canvas.copy(), tiles, yx, 3, opacity=256)


@pytest.mark.parametrize("on_white", [False, True])
@pytest.mark.parametrize("k", [1, 2, 3, 4, 8, 16])
def test_view_restatement_against_a_loop(k, on_white):
    canvas = cr.view_canvas()
    got = painting.canvas_view_numpy(canvas, *cr.VIEW_WINDOW, k, on_white)
    want = cr.view_loop(canvas, *cr.VIEW_WINDOW, k, on_white)
    assert got.dtype == np.uint8 and got.shape == want.shape == (-(-117 // k), -(-131 // k), 3 if on_white else 4)
    assert np.array_equal(got, want)
    if k == 16:
        assert (got[2, 3] == (255 if on_white else 0)).all()                     # the all-transparent block
        full = np.full((140, 150, 4), 255, np.uint8)                              # the largest sums
        assert (painting.canvas_view_numpy(full, *cr.VIEW_WINDOW, 16, on_white) == 255).all()
        assert np.array_equal(painting.canvas_view_numpy(full, *cr.VIEW_WINDOW, 16, on_white), cr.view_loop(full, *cr.VIEW_WINDOW, 16, on_white))


def test_view_restatement_refuses_bad_arguments():
    canvas = cr.view_canvas()
    for args in ((5, 9, 117, 131, 0), (5, 9, 117, 131, 17), (5, 9, 136, 131, 2), (5, 20, 117, 131, 2), (-1, 9, 10, 10, 2), (5, 9, 0, 10, 1)):
        with pytest.raises(ValueError):
            painting.canvas_view_numpy(canvas, *args)


# ---------------------------------------------------------------------------------------------------------------------
# the entries
# ---------------------------------------------------------------------------------------------------------------------
def test_entries_are_exported_and_bound():
    build.build()
    library = _lib.lib()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "neube_hip.h")).read(), flags=re.S)
    for name, n_args in (("nb_over_tiles_u8", 17), ("nb_canvas_view_u8", 11)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m and len(m.group(1).split(",")) == n_args == len(_lib.PROTOTYPES[name][1]), name
        assert _lib.PROTOTYPES[name][0] is C.c_int and hasattr(library, name)
    common = open(os.path.join(REPO, "brushstroke_engine_amd", "csrc", "nb_common.h")).read()
    assert int(re.search(r"#define NB_ABI_VERSION (\d+)", common).group(1)) == _lib.ABI_VERSION >= 20
    assert library.nb_abi_version() == _lib.ABI_VERSION
    assert "nb_compose.hip" in build.SOURCES
    # the CPU stand-ins inherit the restatements; TileOps overrides them with the kernels
    for name in ("over_tiles", "canvas_view"):
        assert hasattr(painting.TileOpsBase, name) and getattr(painting.TileOps, name) is not getattr(painting.TileOpsBase, name)


def test_entries_validate_before_any_launch():
    """Every refusal is decided on the host (no GPU here): nothing is launched and no pointer is read."""
    build.build()
    library = _lib.lib()
    buf = np.zeros(4096, np.uint8)
    p = buf.ctypes.data + (-buf.ctypes.data) % 16
    E = _lib.NB_EINVAL
    ok = dict(tiles=p, t=1, r=8, dst=p, crop=1, canvas=p, h=16, w=128, off=p, lst=p, cx0=0, cy0=0, ncx=2, ncy=4, mode=0, opacity=255)

    def over(**kw):
        a = dict(ok, **kw)
        return library.nb_over_tiles_u8(a["tiles"], a["t"], a["r"], a["dst"], a["crop"], a["canvas"], a["h"], a["w"], a["off"], a["lst"],
                                        a["cx0"], a["cy0"], a["ncx"], a["ncy"], a["mode"], a["opacity"], None)
    for bad in (dict(tiles=None), dict(dst=None), dict(canvas=None), dict(off=None), dict(lst=None), dict(t=0), dict(r=0), dict(h=0), dict(w=-1),
                dict(crop=-1), dict(crop=4), dict(mode=2), dict(mode=-1), dict(opacity=256), dict(opacity=-1), dict(ncx=0), dict(ncy=0),
                dict(cx0=-1), dict(cy0=-1), dict(cx0=1, ncx=2), dict(cy0=3, ncy=2), dict(canvas=p + 2), dict(tiles=p + 1)):
        assert over(**bad) == E, bad
        assert b"over_tiles" in library.nb_last_error()

    def view(canvas=p, ch=20, cw=30, y0=2, x0=3, h=18, w=27, k=4, on_white=0, out=p):
        return library.nb_canvas_view_u8(canvas, ch, cw, y0, x0, h, w, k, on_white, out, None)
    for bad in (dict(canvas=None), dict(out=None), dict(ch=0), dict(cw=0), dict(h=0), dict(w=0), dict(k=0), dict(k=17), dict(on_white=2),
                dict(on_white=-1), dict(y0=-1), dict(x0=-1), dict(h=19), dict(w=28), dict(canvas=p + 2), dict(out=p + 2)):
        assert view(**bad) == E, bad
        assert b"canvas_view" in library.nb_last_error()


# ---------------------------------------------------------------------------------------------------------------------
# the session on the oracle-backed ops
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracle_ops():
    g = load_golden("engine_r128.npz")
    cfg = cfgmod.style1_config(int(g["resolution"]))
    ops = OracleTileOps(cfg, wmod.random_state_dict(cfg, seed=int(g["weights_seed"])), encmod.random_encoder_state_dict(int(g["encoder_seed"])))
    return ops, int(g["crop_margin"])


@pytest.mark.parametrize("level", [0, 2])
def test_session_on_the_oracle_ops(oracle_ops, level):
    ops, m = oracle_ops
    with torch.no_grad():
        session = cr.check_session(ops, level, m, lambda t: t.numpy())
        # erase with the same strokes at half opacity: alpha goes down where the stroke is, colours stay
        before = session.canvas.numpy().copy()
        session.add(cr.session_strokes()[0], cr.session_brushes(ops.cfg.z_dim)[0], mode="erase", opacity=128)
        after = session.canvas.numpy()
        assert np.array_equal(after[..., :3], before[..., :3]) and (after[..., 3] <= before[..., 3]).all() and (after[..., 3] < before[..., 3]).any()
        assert session.undo() != painting.EMPTY_BOX and np.array_equal(session.canvas.numpy(), before)
        assert session.undo() != painting.EMPTY_BOX and not session.canvas.numpy().any()
        assert session.undo() == painting.EMPTY_BOX
        for bad in (dict(mode="multiply"), dict(opacity=256), dict(opacity=-1), dict(opacity=1.5)):
            with pytest.raises(ValueError):
                session.add(cr.session_strokes()[0], cr.session_brushes(ops.cfg.z_dim)[0], **bad)
    with pytest.raises(ValueError):
        painting.PaintSession(painting.PaintingHelper(ops), (0, 10))


def test_strokes_bounds_contain_the_raster():
    """The host's box holds every stroke pixel the float64 rasteriser draws, spline overshoot included."""
    strokes = painting.StrokeList().add_spline([[20.0, 20.0], [60.0, 22.0], [62.0, 70.0], [30.0, 65.0]], 2.5, through_ends=False)
    strokes.add_polyline([[80.5, 90.0]], 7.0)
    y0, x0, y1, x1 = painting.strokes_bounds(strokes)
    ys, xs = np.nonzero(painting.raster_strokes_numpy(strokes, (120, 120)) == 0)
    assert y0 <= ys.min() and x0 <= xs.min() and y1 > ys.max() and x1 > xs.max() and len(ys) > 100
    assert y1 - y0 < 100 and x1 - x0 < 100                                            # ... and is no whole-canvas answer
    assert painting.strokes_bounds(painting.StrokeList()) is None


# ---------------------------------------------------------------------------------------------------------------------
# the script of paint_session_main
# ---------------------------------------------------------------------------------------------------------------------
def test_script_parsing():
    import json
    s = paint_session_main.parse_script(json.dumps(cr.good_script()))
    assert s["size"] == (150, 150) and s["crop_margin"] == 10 and s["feature_blending_level"] == 2 and len(s["layers"]) == 2
    a, b = s["layers"]
    assert (a["mode"], a["opacity"], a["colors"], a["library"], a["style_id"]) == ("paint", 255, [], "594,12", "594") and len(a["strokes"]) == 2
    assert (b["mode"], b["opacity"], b["colors"]) == ("erase", 128, [[200, 30, 40], None, [20, 60, 220]])
    opts = paint_session_main.layer_options(b, {}, 64)
    assert opts.style_id == "12" and opts.color1 is None and torch.allclose(opts.color0, torch.tensor([[200, 30, 40]]) / 255.0)
    minimal = paint_session_main.parse_script({"size": [5, 7], "layers": [{"strokes": [], "style_id": 3}]})
    assert (minimal["crop_margin"], minimal["feature_blending_level"], minimal["layers"][0]["library"]) == (10, 0, "rand100")

    def broken(**kw):
        s = cr.good_script()
        for key, v in kw.items():
            if key.startswith("layer_"):
                s["layers"][1][key[6:]] = v
            else:
                s[key] = v
        return s
    for bad in (broken(layer_mode="multiply"), broken(layer_mode=1), broken(layer_opacity=256), broken(layer_opacity=-1),
                broken(layer_opacity=0.5), broken(layer_opacity="255"), broken(size=[0, 150]), broken(size=[150]), broken(size=[150, -2]),
                broken(size="150,150"), broken(size=[150.5, 150]), broken(layers=[]), broken(layers=None), broken(crop_margin=-1),
                broken(layer_colors=[[1, 2]]), broken(layer_colors=[[1, 2, 300]]), broken(layer_strokes=[{"type": "circle"}]), [1, 2]):
        with pytest.raises(ValueError):
            paint_session_main.parse_script(bad)
    with pytest.raises(SystemExit):
        paint_session_main.build_parser().parse_args(["--gan_checkpoint", "e.npz", "--script", "s.json"])        # no output prefix
