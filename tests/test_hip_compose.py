"""The compositing kernels (csrc/nb_compose.hip) through ctypes against their numpy restatements, byte for byte -- both are exact
integer arithmetic --, ``painting.PaintSession`` on ``TileOps`` against ``paint_strokes``, and the command line of
``paint_session_main``.  Output buffers sit between guard bytes that must survive."""
import json

import numpy as np
import pytest
import torch

import compose_refs as cr
from conftest import load_golden
from brushstroke_engine_amd import _lib, config as cfgmod, encoder as encmod, painting, weights as wmod

pytestmark = pytest.mark.gpu

GUARD = 256              # bytes of 0xA5 on either side of a guarded buffer


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _guarded(a, lead=0):
    """``a`` (numpy uint8) on the device, GUARD + lead bytes into an allocation filled with 0xA5 -> (allocation, pointer, byte count).
    lead = 0 keeps the 16-byte alignment of the allocation; lead = 4 leaves only the 4-byte alignment the entries ask for."""
    buf = torch.full([GUARD + lead + a.size + GUARD], 0xA5, dtype=torch.uint8, device="cuda")
    buf[GUARD + lead:GUARD + lead + a.size].copy_(_dev(a.reshape(-1)))
    return buf, buf.data_ptr() + GUARD + lead, a.size


def _unguard(buf, lead, shape):
    host = buf.cpu().numpy()
    n = int(np.prod(shape))
    assert (host[:GUARD + lead] == 0xA5).all() and (host[GUARD + lead + n:] == 0xA5).all(), "wrote outside the buffer"
    return host[GUARD + lead:GUARD + lead + n].reshape(shape)


def _over(tiles, yx, crop, canvas, box=None, mode=0, opacity=255, lead=0):
    """nb_over_tiles_u8 through ctypes on a guarded canvas -> the canvas as numpy."""
    h, w = canvas.shape[:2]
    r = tiles.shape[1]
    rects = np.concatenate([yx + crop, yx + r - crop], axis=1)
    off, lst = painting.build_cells(rects, h, w)
    cells = painting.cell_box(box, h, w)
    buf, ptr, _ = _guarded(canvas, lead)
    d_tiles, d_yx, d_off, d_lst = _dev(tiles), _dev(yx.astype(np.int32)), _dev(off), _dev(lst)
    _lib.check(_lib.lib().nb_over_tiles_u8(d_tiles.data_ptr(), tiles.shape[0], r, d_yx.data_ptr(), crop, ptr, h, w, d_off.data_ptr(),
                                           d_lst.data_ptr(), *cells, mode, opacity, _stream()), "over_tiles")
    torch.cuda.synchronize()
    return _unguard(buf, lead, canvas.shape)


# ---------------------------------------------------------------------------------------------------------------------
# nb_over_tiles_u8
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lead", [0, 4], ids=["vectors", "pixels"])
@pytest.mark.parametrize("mode", [0, 1], ids=["paint", "erase"])
def test_over_every_alpha_pair(mode, lead):
    """All 256 x 256 (source alpha, destination alpha) pairs at four opacities and four colour pairs: one tile with crop 0."""
    for cs, cd in cr.COLOUR_PAIRS:
        tile, canvas = cr.alpha_square(cs, cd)
        for opacity in cr.OPACITIES:
            got = _over(tile, np.zeros((1, 2), np.int64), 0, canvas, None, mode, opacity, lead)
            want = painting.over_tiles_numpy(canvas.copy(), tile, [[0, 0]], 0, mode, opacity)
            bad = np.argwhere((got != want).any(axis=2))
            assert len(bad) == 0, (cs, cd, opacity, bad[:4].tolist(), got[tuple(bad[0])].tolist(), want[tuple(bad[0])].tolist())


@pytest.mark.parametrize("h,w,lead", [(117, 131, 0), (117, 131, 4), (117, 132, 0), (117, 132, 4)],
                         ids=["131-pixels", "131-pixels-unaligned", "132-vectors", "132-pixels-unaligned"])
@pytest.mark.parametrize("mode,opacity", [(0, 255), (0, 77), (1, 200)])
def test_over_seven_tiles(h, w, lead, mode, opacity):
    """Overlapping interiors, negative origins, a tile over the far edge, a box smaller than the tiles' extent: the last interior
    is the source, and covered pixels outside the box keep their bytes like everything else."""
    tiles, yx, crop, canvas, box = cr.over_scene(h, w)
    cells = painting.cell_box(box, h, w)
    want = painting.over_tiles_numpy(canvas.copy(), tiles, yx, crop, mode, opacity, cells)
    everywhere = painting.over_tiles_numpy(canvas.copy(), tiles, yx, crop, mode, opacity)
    assert not np.array_equal(want, everywhere) and not np.array_equal(want, canvas)          # the box does cut covered pixels off
    got = _over(tiles, yx.astype(np.int64), crop, canvas, box, mode, opacity, lead)
    assert np.array_equal(got, want)
    assert np.array_equal(_over(tiles, yx.astype(np.int64), crop, canvas, box, mode, opacity, lead), got)      # run to run
    assert np.array_equal(_over(tiles, yx.astype(np.int64), crop, canvas, None, mode, opacity, lead), everywhere)


def test_over_refuses_without_a_launch():
    tiles, yx, crop, canvas, box = cr.over_scene()
    h, w = canvas.shape[:2]
    off, lst = painting.build_cells(np.concatenate([yx + crop, yx + 40 - crop], axis=1), h, w)
    buf, ptr, _ = _guarded(canvas)
    d_tiles, d_yx, d_off, d_lst = _dev(tiles), _dev(yx), _dev(off), _dev(lst)
    ok = dict(tiles=d_tiles.data_ptr(), t=7, r=40, dst=d_yx.data_ptr(), crop=crop, canvas=ptr, h=h, w=w, off=d_off.data_ptr(),
              lst=d_lst.data_ptr(), cx0=0, cy0=0, ncx=3, ncy=30, mode=0, opacity=255)
    lib = _lib.lib()
    for bad in (dict(tiles=None), dict(dst=None), dict(canvas=None), dict(off=None), dict(lst=None), dict(t=0), dict(r=0), dict(h=0), dict(w=0),
                dict(crop=-1), dict(crop=20), dict(mode=2), dict(mode=-1), dict(opacity=256), dict(opacity=-1), dict(ncx=0), dict(ncy=0),
                dict(cx0=-1), dict(cy0=-1), dict(cx0=1), dict(cy0=1), dict(ncx=4), dict(ncy=31), dict(canvas=ptr + 2)):
        a = dict(ok, **bad)
        rc = lib.nb_over_tiles_u8(a["tiles"], a["t"], a["r"], a["dst"], a["crop"], a["canvas"], a["h"], a["w"], a["off"], a["lst"], a["cx0"],
                                  a["cy0"], a["ncx"], a["ncy"], a["mode"], a["opacity"], _stream())
        assert rc == _lib.NB_EINVAL, bad
    torch.cuda.synchronize()
    assert np.array_equal(_unguard(buf, 0, canvas.shape), canvas)                         # nothing ran


# ---------------------------------------------------------------------------------------------------------------------
# nb_canvas_view_u8
# ---------------------------------------------------------------------------------------------------------------------
def _view(canvas, y0, x0, h, w, k, on_white, lead=0):
    ch, cw = canvas.shape[:2]
    cbuf, cptr, _ = _guarded(canvas, lead)
    shape = (-(-h // k), -(-w // k), 3 if on_white else 4)
    obuf, optr, _ = _guarded(np.full(shape, 0x5A, np.uint8))
    _lib.check(_lib.lib().nb_canvas_view_u8(cptr, ch, cw, y0, x0, h, w, k, int(on_white), optr, _stream()), "canvas_view")
    torch.cuda.synchronize()
    assert np.array_equal(_unguard(cbuf, lead, canvas.shape), canvas)                     # the canvas is only read
    return _unguard(obuf, 0, shape)


@pytest.fixture(scope="module")
def view_wants():
    """The restatement at the cases of tests/test_compose_cpu.py (which holds it to the loop), computed once."""
    canvas = cr.view_canvas()
    return canvas, {(k, w): painting.canvas_view_numpy(canvas, *cr.VIEW_WINDOW, k, w) for k in (1, 2, 3, 4, 8, 16) for w in (False, True)}


@pytest.mark.parametrize("on_white", [False, True])
@pytest.mark.parametrize("k", [1, 2, 3, 4, 8, 16])
def test_view_window(view_wants, k, on_white):
    canvas, wants = view_wants                                        # 150 wide: one pixel per lane
    assert np.array_equal(_view(canvas, *cr.VIEW_WINDOW, k, on_white), wants[(k, on_white)])
    wide = np.concatenate([canvas, canvas[:, :2]], axis=1)             # 152 wide: 16-byte vectors, the window still starts at column 9
    assert np.array_equal(_view(wide, *cr.VIEW_WINDOW, k, on_white), wants[(k, on_white)])
    assert np.array_equal(_view(wide, *cr.VIEW_WINDOW, k, on_white, lead=4), wants[(k, on_white)])       # unaligned: pixels again
    if k == 16:
        full = np.full((140, 152, 4), 255, np.uint8)
        assert (_view(full, *cr.VIEW_WINDOW, 16, on_white) == 255).all()


@pytest.mark.parametrize("cw", [2600, 2601], ids=["vectors", "pixels"])
@pytest.mark.parametrize("k", [1, 3, 16])
def test_view_over_several_strips(cw, k):
    """A window wider than what one workgroup's lanes load (1021 / k output columns with vectors, 256 / k without), with a clipped
    last block in both directions and more rows than one workgroup takes."""
    canvas = cr.view_canvas(41, cw, seed=2)
    for on_white in (False, True):
        assert np.array_equal(_view(canvas, 2, 7, 38, 2590, k, on_white), painting.canvas_view_numpy(canvas, 2, 7, 38, 2590, k, on_white))


def test_view_refuses_without_a_launch():
    canvas = cr.view_canvas()
    cbuf, cptr, _ = _guarded(canvas)
    shape = (30, 33, 4)
    obuf, optr, _ = _guarded(np.full(shape, 0x5A, np.uint8))
    ok = dict(canvas=cptr, ch=140, cw=150, y0=5, x0=9, h=117, w=131, k=4, on_white=0, out=optr)
    for bad in (dict(canvas=None), dict(out=None), dict(ch=0), dict(cw=0), dict(h=0), dict(w=0), dict(k=0), dict(k=17), dict(on_white=2),
                dict(y0=-1), dict(x0=-1), dict(h=136), dict(w=142), dict(canvas=cptr + 1), dict(out=optr + 2)):
        a = dict(ok, **bad)
        rc = _lib.lib().nb_canvas_view_u8(a["canvas"], a["ch"], a["cw"], a["y0"], a["x0"], a["h"], a["w"], a["k"], a["on_white"], a["out"],
                                          _stream())
        assert rc == _lib.NB_EINVAL, bad
    torch.cuda.synchronize()
    assert (_unguard(obuf, 0, shape) == 0x5A).all()                                       # nothing ran


# ---------------------------------------------------------------------------------------------------------------------
# the session
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    """The engine_r128 job with its seeded network, as tests/test_hip_stroke_raster.py sets it up."""
    g = load_golden("engine_r128.npz")
    cfg = cfgmod.style1_config(128)
    sd = wmod.random_state_dict(cfg, seed=0)
    esd = encmod.random_encoder_state_dict(5)
    from brushstroke_engine_amd.networks import Generator
    G = Generator(cfg, sd, conv_mode="h3").to("cuda")
    ops = painting.TileOps(G, encmod.HipGeometryEncoder(esd))
    return dict(ops=ops, cfg=cfg, sd=sd, esd=esd, m=int(g["crop_margin"]))


@pytest.mark.parametrize("level", [0, 2])
def test_session_on_tileops(eng, level):
    """One add equals paint_strokes, a second brush goes over it as the restatement says, undo gives the first back; the view of
    the session equals the restatement on the downloaded canvas (all of it inside compose_refs.check_session)."""
    with torch.no_grad():
        session = cr.check_session(eng["ops"], level, eng["m"], lambda t: t.cpu().numpy())
    assert session.canvas.is_cuda and session.canvas.data_ptr() % 16 == 0 and session.canvas.shape[1] % 4 == 0     # the vector path


def test_session_main_writes_what_the_api_gives(eng, tmp_path):
    from PIL import Image
    from brushstroke_engine_amd import formats, paint_session_main
    snap = str(tmp_path / "engine.npz")
    formats.save_engine_snapshot(snap, eng["cfg"], eng["sd"], eng["esd"], preproc_type=None)
    script = tmp_path / "session.json"
    script.write_text(json.dumps(cr.good_script()))
    written = paint_session_main.main(["--gan_checkpoint", snap, "--script", str(script), "--output_file_prefix", str(tmp_path / "cli" / "res"),
                                       "--on_white", "--conv_mode", "h3"])
    assert written == str(tmp_path / "cli" / "res") + ".png"
    first, second, _ = cr.session_strokes()
    brush_a, brush_b = cr.session_brushes(eng["cfg"].z_dim)
    brush_b.set_color(1, None)                                         # the script's second layer: primary and canvas colour
    brush_b.set_color(2, np.array([20, 60, 220], np.uint8))
    brush_a.style_id, brush_b.style_id = "594", "12"
    helper = painting.PaintingHelper(eng["ops"])
    helper.set_feature_blending(2)
    session = painting.PaintSession(helper, cr.SIZE, crop_margin=10)
    with torch.no_grad():
        session.add(first, brush_a)
        session.add(second, brush_b, mode="erase", opacity=128)
    mine = str(tmp_path / "mine.png")
    Image.fromarray(session.image(on_white=True)).save(mine)
    assert open(written, "rb").read() == open(mine, "rb").read()
    img = np.array(Image.open(written))
    assert img.shape == (150, 150, 3) and (img < 255).any()
