"""Drawing preparation on the device (csrc/nb_geomprep.hip) against the host code it replaces: the numpy functions
``prepare_geometry_image`` / ``pad_geo`` / ``generate_stitching_crops`` and the torch on-white expression of ``paint_image``.
Every comparison is exact equality: one threshold step flips whole regions of a drawing."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from brushstroke_engine_amd import _lib, config as cfgmod, encoder as encmod, painting, weights as wmod

pytestmark = pytest.mark.gpu

EINVAL = _lib.NB_EINVAL


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _new_ws():
    # garbage on purpose: the entry clears its own scratch
    return torch.full([_lib.NB_GEOM_PREP_WS_BYTES // 4], 0x5A5A5A5A, dtype=torch.int32, device="cuda")


def _prepare(img, out_shape=None, offset=(0, 0), ws=None):
    """nb_geom_prepare_u8 through ctypes -> (out [out_h,out_w] numpy, scratch words numpy)."""
    h, w = img.shape[:2]
    ch = 1 if img.ndim == 2 else img.shape[2]
    oh, ow = (h, w) if out_shape is None else out_shape
    d_img = _dev(img)
    out = torch.full([oh, ow], 77, dtype=torch.uint8, device="cuda")
    ws = _new_ws() if ws is None else ws
    rc = _lib.lib().nb_geom_prepare_u8(d_img.data_ptr(), h, w, ch, out.data_ptr(), oh, ow, offset[0], offset[1], ws.data_ptr(), _stream())
    _lib.check(rc, "geom_prepare")
    torch.cuda.synchronize()
    return out.cpu().numpy(), ws.cpu().numpy().view(np.uint32)


def _want(img, out_shape=None, offset=(0, 0)):
    """The parent's numpy route: thresholded drawing at `offset` of a 255 buffer."""
    g = painting.prepare_geometry_image(img)[..., 0]
    if out_shape is None:
        return g
    out = np.full(out_shape, 255, np.uint8)
    out[offset[0]:offset[0] + g.shape[0], offset[1]:offset[1] + g.shape[1]] = g
    return out


def _gray8(img):
    """The stretched uint8 image prepare_geometry_image thresholds (its histogram is what the scratch holds)."""
    a = np.asarray(img).astype(np.float32)
    if a.ndim == 2:
        a = a[..., None]
    if a.shape[2] == 3:
        a = a.mean(axis=2, dtype=np.float32)
    elif a.shape[2] == 4:
        mean = a[..., :3].mean(axis=2, dtype=np.float32)
        alpha = a[..., 3] / np.float32(255)
        a = mean * alpha + np.float32(255) * (1 - alpha)
    mn = a.min()
    if mn > 0:
        a = a - mn
    mx = a.max()
    if 0 < mx < 255:
        a = a * np.float32(255.0 / float(mx))
    return a.astype(np.uint8)


def _check(img):
    """Equal to numpy at offset (0, 0) and at an offset inside a larger buffer; the scratch holds the histogram and threshold."""
    h, w = img.shape[:2]
    got, ws = _prepare(img)
    want = _want(img)
    assert np.array_equal(got, want), (np.argwhere(got != want)[:4], ws[:3])
    shape, off = (h + 13, w + 22), (5, 9)
    got2, _ = _prepare(img, shape, off)
    assert np.array_equal(got2, _want(img, shape, off))
    g8 = _gray8(img)
    assert np.array_equal(ws[4:260], np.bincount(g8.ravel(), minlength=256))
    assert int(ws[4:260].sum()) == h * w
    assert float(ws[2]) == painting.threshold_otsu(g8)
    return got, ws


def _strokes(h, w, seed, lo=0, hi=256, channels=3):
    rs = np.random.RandomState(seed)
    return rs.randint(lo, hi, (h, w) if channels == 1 else (h, w, channels)).astype(np.uint8)


@pytest.mark.parametrize("channels", [1, 3, 4])
def test_prepare_odd_size(channels):
    """37 x 53 divides no block shape: everything is in one ragged workgroup and the 4-pixel tail."""
    out, _ = _check(_strokes(37, 53, channels, channels=channels))
    assert set(np.unique(out)) == {0, 255}


def test_prepare_several_workgroups():
    """601 x 700 x 3: hundreds of workgroups, a ragged last one, 601 * 700 % 4 == 0 but rows that start at odd byte offsets."""
    _check(_strokes(601, 700, 11))
    _check(_strokes(601, 699, 12))                  # npix % 4 == 3: the scalar tail


def test_prepare_all_channel_sums():
    """Every r + g + b in 0..765 (each /3 must round like numpy's fp32 division)."""
    s = np.arange(766)
    r = np.minimum(s, 255)
    g = np.minimum(s - r, 255)
    b = s - r - g
    img = np.stack([r, g, b], 1).astype(np.uint8)
    assert np.array_equal(img.astype(np.int64).sum(1), s)
    img = np.concatenate([img, img[::-1][:2]]).reshape(24, 32, 3)          # 768 pixels
    _check(img)
    _check(np.ascontiguousarray(img[..., ::-1]))


def test_prepare_all_alphas_against_means():
    """All 256 alphas against a spread of 50 channel sums (means with all three fractional parts)."""
    sums = np.unique(np.concatenate([np.arange(0, 766, 17), [1, 2, 383, 764, 765]]))
    assert len(sums) == 50
    img = np.zeros((256, len(sums), 4), np.uint8)
    for j, s in enumerate(sums):
        r = min(s, 255)
        g = min(s - r, 255)
        img[:, j, :3] = (r, g, s - r - g)
    img[..., 3] = np.arange(256)[:, None]
    _check(img)


def test_prepare_min_above_zero():
    """mn > 0 and nothing to scale afterwards.  uint8 input keeps max - min below 255 whenever min > 0, so the subtraction runs
    alone only where it leaves a maximum of 0: constant drawings above 0, at 1, 3 and 4 channels (fractional minima included)."""
    for px in [(128,), (9, 9, 10), (200, 201, 202, 77), (1, 0, 0, 255)]:
        img = np.empty((19, 23, len(px)) if len(px) > 1 else (19, 23), np.uint8)
        img[...] = px if len(px) > 1 else px[0]
        assert float(_gray8(img).max()) == 0 and painting.prepare_geometry_image(img).max() == 0
        out, ws = _check(img)
        assert ws[0] == ws[1] > 0 and (out == 0).all()              # min == max > 0 in the scratch


def test_prepare_max_below_255():
    img = _strokes(40, 44, 5, lo=0, hi=200)
    img[0, 0], img[1, 1] = 0, 199                    # mn = 0: no subtraction; 0 < mx = 199 < 255: scaling
    _check(img[..., 0])
    img[0, 0] = (0, 0, 0)
    img[1, 1] = (199, 199, 198)                      # fractional maximum 198.66667
    _check(img)
    rgba = _strokes(33, 35, 6, lo=0, hi=120, channels=4)
    rgba[..., 3] = 255                               # opaque: gray = mean * 1 + 255 * 0
    rgba[0, 0, :3] = 0
    _check(rgba)


def test_prepare_subtract_and_scale():
    img = _strokes(39, 45, 7, lo=30, hi=181)
    img[0, 0], img[1, 1] = (30, 30, 31), (180, 180, 179)
    _check(img)                                      # mn = 30.333334 > 0, then 0 < mx - mn < 255
    _check(np.ascontiguousarray(img[..., 1]))


@pytest.mark.parametrize("value", [0, 1, 128, 255])
def test_prepare_constant_image(value):
    """lo == hi: the threshold is that value and nothing exceeds it."""
    for ch in (1, 3):
        img = np.full((21, 30) if ch == 1 else (21, 30, ch), value, np.uint8)
        out, ws = _check(img)
        assert (out == 0).all() and ws[4:260].max() == 21 * 30


def test_prepare_two_values():
    """The smallest occupied range (a single candidate) and equal class sizes; neighbouring values; the far ends."""
    for a, b in [(0, 255), (254, 255), (0, 1), (100, 101), (7, 200)]:
        img = np.full((24, 24), a, np.uint8)
        img[:, 12:] = b
        out, ws = _check(img)
        assert (out[:, :12] == 0).all() and (out[:, 12:] == 255).all()
    img = np.repeat(np.array([0, 85, 170, 255], np.uint8), 5)[None, :].repeat(16, 0)      # four equally filled, equally spaced values:
    _, ws = _check(img)                                                                  # var12 has the same maximum on all of 85..169
    assert ws[2] == 85                                                                   # the first one
    img = np.zeros((16, 16), np.uint8)               # symmetric histogram 0 / 128 (empty) / 255: a plateau of equal maxima
    img[:, 8:] = 255
    _check(img)


def test_prepare_near_constant_drawing():
    """A white sheet with < 1 % dark pixels: every lane of the histogram pass folds one long run; the counts must be complete."""
    h, w = 512, 640
    img = np.full((h, w, 3), 255, np.uint8)
    img[100:103, 50:600] = 0
    img[200:420, 300:302] = (10, 20, 30)
    assert (img[..., 0] < 255).mean() < 0.01
    out, ws = _check(img)
    assert int(ws[4:260].sum()) == h * w and ws[4 + 255] == (img[..., 0] == 255).sum()
    assert (out[100:103, 50:600] == 0).all()


def test_prepare_reuses_scratch():
    """Two calls on one ws: the second must not see the first call's extrema or counts."""
    ws = _new_ws()
    a = _strokes(50, 60, 20)                         # full range
    b = _strokes(35, 31, 21, lo=90, hi=140)          # narrower than a's extrema on both ends, fewer pixels
    got_a, _ = _prepare(a, ws=ws)
    got_b, words = _prepare(b, ws=ws)
    assert np.array_equal(got_a, _want(a)) and np.array_equal(got_b, _want(b))
    assert int(words[4:260].sum()) == 35 * 31
    got_a2, _ = _prepare(a, ws=ws)
    assert np.array_equal(got_a2, got_a)


def test_prepare_rejects_bad_arguments():
    """Every NB_EINVAL case leaves `out` untouched."""
    lib = _lib.lib()
    img = _dev(_strokes(8, 10, 1))
    out = torch.full([12, 14], 77, dtype=torch.uint8, device="cuda")
    ws = _new_ws()

    def call(img_p=img.data_ptr(), h=8, w=10, ch=3, out_p=out.data_ptr(), oh=12, ow=14, oy=2, ox=3, ws_p=ws.data_ptr()):
        return lib.nb_geom_prepare_u8(img_p, h, w, ch, out_p, oh, ow, oy, ox, ws_p, _stream())
    for bad in (dict(ch=0), dict(ch=2), dict(ch=5), dict(img_p=None), dict(out_p=None), dict(ws_p=None), dict(oy=5), dict(ox=5),
                dict(oy=-1), dict(ox=-1), dict(oh=9), dict(ow=12), dict(h=0), dict(w=0)):
        assert call(**bad) == EINVAL, bad
        assert lib.nb_last_error()
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 77).all()
    assert call() == 0                               # the good call of the same shape does write
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), _want(img.cpu().numpy(), (12, 14), (2, 3)))


def test_prepare_graph_replay():
    """One call captured into a hipGraph (enqueue-only: no allocation, synchronisation or read-back inside) == the eager call."""
    a, b = _strokes(90, 75, 30, channels=4), _strokes(90, 75, 31, lo=20, hi=230, channels=4)
    shape, off = (120, 100), (10, 10)
    img = _dev(a)
    out = torch.zeros(shape, dtype=torch.uint8, device="cuda")
    ws = _new_ws()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                    # load the code objects before the capture
        _lib.check(_lib.lib().nb_geom_prepare_u8(img.data_ptr(), 90, 75, 4, out.data_ptr(), *shape, *off, ws.data_ptr(), side.cuda_stream), "warm")
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _lib.check(_lib.lib().nb_geom_prepare_u8(img.data_ptr(), 90, 75, 4, out.data_ptr(), *shape, *off, ws.data_ptr(), _stream()), "capture")
    for drawing in (b, a):
        img.copy_(_dev(drawing))
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        eager, _ = _prepare(drawing, shape, off)
        assert np.array_equal(out.cpu().numpy(), eager)
        assert np.array_equal(eager, _want(drawing, shape, off))


# ---------------------------------------------------------------------------------------------------------------------
# tile picks
# ---------------------------------------------------------------------------------------------------------------------
def _tile_geometry():
    """300 x 280, R = 128, stride 88: 4 x 4 tiles, the last row / column hang over the edge.  Tile (0, 0) holds exactly 10 stroke
    pixels, tiles (0, 2) and (0, 3) exactly 11, (3, 3) [rows and columns from 264: 36 x 16 pixels inside] the image corner."""
    geom = np.full((300, 280), 255, np.uint8)
    geom[3, 2:12] = 0                                 # 10 pixels, columns < 88: tile (0, 0) only
    geom[5, 266:277] = 0                              # 11 pixels, columns >= 264: tiles (0, 2) [176..303] and (0, 3) [264..]
    geom[150:160, 100:140] = 0                        # a block inside several overlapping tiles
    geom[290:300, 270:280] = 0                        # the image corner: windows hanging over both edges
    geom[200, 30] = 1                                 # not a stroke pixel (only == 0 counts)
    return geom


def _numpy_counts(geom, r, stride, nrows, ncols):
    padded = np.full((nrows * stride + r, ncols * stride + r), 255, np.uint8)
    padded[:geom.shape[0], :geom.shape[1]] = geom
    return np.array([[np.sum(padded[y * stride:y * stride + r, x * stride:x * stride + r] < 0.001) for x in range(ncols)]
                     for y in range(nrows)], np.int32)


def test_tile_stroke_counts():
    geom = _tile_geometry()
    r, stride = 128, 88
    nrows, ncols = 300 // stride + 1, 280 // stride + 1
    want = _numpy_counts(geom, r, stride, nrows, ncols)
    assert want[0, 0] == 10 and want[0, 3] == 11 and want[3, 3] == 100 and (nrows, ncols) == (4, 4)
    assert (nrows - 1) * stride + r > 300 and (ncols - 1) * stride + r > 280          # windows hang over the edges
    counts = torch.full([nrows, ncols], -1, dtype=torch.int32, device="cuda")
    g = _dev(geom)
    _lib.check(_lib.lib().nb_tile_stroke_counts_u8(g.data_ptr(), 300, 280, r, stride, nrows, ncols, counts.data_ptr(), _stream()), "counts")
    assert np.array_equal(counts.cpu().numpy(), want)
    # a grid that reaches past the image altogether: windows with no pixel inside count nothing
    counts = torch.full([6, 5], -1, dtype=torch.int32, device="cuda")
    _lib.check(_lib.lib().nb_tile_stroke_counts_u8(g.data_ptr(), 300, 280, r, stride, 6, 5, counts.data_ptr(), _stream()), "counts")
    assert np.array_equal(counts.cpu().numpy(), _numpy_counts(geom, r, stride, 6, 5))
    assert (counts.cpu().numpy()[4:] == 0).all()
    # the kept tiles: count > 10, as generate_stitching_crops picks them
    crops, _ = painting.generate_stitching_crops(geom[..., None], r, "stroke", (r - stride) // 2)
    kept = [(y * stride, x * stride, r, r) for y in range(nrows) for x in range(ncols) if want[y, x] > 10]
    assert kept == crops and (0, 0, r, r) not in crops and (0, 3 * stride, r, r) in crops


# ---------------------------------------------------------------------------------------------------------------------
# crop + on-white
# ---------------------------------------------------------------------------------------------------------------------
def _torch_on_white(canvas, y0, x0, h, w):
    """The expression of PaintingHelper.paint_image (alpha through a host-computed table)."""
    result = canvas[y0:y0 + h, x0:x0 + w]
    lut = _dev(np.arange(256, dtype=np.float32) / np.float32(255))
    a = lut[result[..., 3:].to(torch.int64)]
    return (result[..., :3].to(torch.float32) * a + 255 * (1 - a)).clip(0, 255).to(torch.uint8)


def _on_white(canvas, y0, x0, h, w):
    out = torch.full([h, w, 3], 77, dtype=torch.uint8, device="cuda")
    ch, cw = canvas.shape[:2]
    _lib.check(_lib.lib().nb_composite_on_white_u8(canvas.data_ptr(), ch, cw, y0, x0, h, w, out.data_ptr(), _stream()), "on_white")
    return out


def test_composite_on_white_all_pairs():
    """256 x 256: row = alpha, column = colour, in all three channels (shifted against each other)."""
    c = np.arange(256, dtype=np.uint8)
    canvas = np.zeros((256, 256, 4), np.uint8)
    canvas[..., 0], canvas[..., 1], canvas[..., 2] = c[None, :], c[None, ::-1], np.roll(c, 77)[None, :]
    canvas[..., 3] = c[:, None]
    d = _dev(canvas)
    assert torch.equal(_on_white(d, 0, 0, 256, 256), _torch_on_white(d, 0, 0, 256, 256))


def test_composite_on_white_window():
    canvas = _dev(_strokes(203, 157, 40, channels=4))
    for (y0, x0, h, w) in [(10, 10, 180, 130), (0, 0, 203, 157), (202, 156, 1, 1), (7, 3, 33, 151)]:
        assert torch.equal(_on_white(canvas, y0, x0, h, w), _torch_on_white(canvas, y0, x0, h, w)), (y0, x0, h, w)
    lib = _lib.lib()
    out = torch.full([4, 4, 3], 77, dtype=torch.uint8, device="cuda")
    for (y0, x0, h, w) in [(200, 0, 4, 4), (0, 154, 4, 4), (-1, 0, 4, 4), (0, 0, 0, 4)]:
        assert lib.nb_composite_on_white_u8(canvas.data_ptr(), 203, 157, y0, x0, h, w, out.data_ptr(), _stream()) == EINVAL
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 77).all()


# ---------------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    """The engine_r128 job with its seeded network, as tests/test_hip_painting.py sets it up."""
    g = load_golden("engine_r128.npz")
    cfg = cfgmod.style1_config(128)
    sd = wmod.random_state_dict(cfg, seed=0)
    esd = encmod.random_encoder_state_dict(5)
    z = np.random.RandomState(594).randn(1, cfg.z_dim)
    from brushstroke_engine_amd.networks import Generator
    G = Generator(cfg, sd, conv_mode="h3").to("cuda")
    ops = painting.TileOps(G, encmod.HipGeometryEncoder(esd))
    geom = g["geom"]
    rgba = np.zeros(geom.shape + (4,), np.uint8)     # opaque black strokes on transparent, as tests/test_painting_cpu.py draws
    rgba[..., 3] = 255 - geom
    return dict(g=g, ops=ops, z=z, rgba=rgba, cfg=cfg, sd=sd, esd=esd)


def test_tileops_wrappers(eng):
    ops, rgba = eng["ops"], eng["rgba"]
    m = int(eng["g"]["crop_margin"])
    h, w = rgba.shape[:2]
    nrows, ncols, stride, ph, pw = painting.stitching_grid(h + m, w + m, 128, 2 * m)
    crops, padded = painting.generate_stitching_crops(painting.pad_geo(painting.prepare_geometry_image(rgba), m), 128, "stroke", 2 * m)
    dev = ops.prepare_geometry(rgba, (ph, pw), (m, m))
    assert np.array_equal(dev.cpu().numpy(), padded[..., 0])
    assert np.array_equal(ops.prepare_geometry(_dev(rgba[..., 3])).cpu().numpy(), painting.prepare_geometry_image(rgba[..., 3])[..., 0])
    counts = ops.stroke_counts(dev, 128, stride, nrows, ncols).cpu().numpy()
    assert np.array_equal(counts, _numpy_counts(padded[..., 0], 128, stride, nrows, ncols))
    canvas = _dev(_strokes(ph, pw, 50, channels=4))
    assert torch.equal(ops.composite_on_white(canvas, m, m, h, w), _torch_on_white(canvas, m, m, h, w))
    with pytest.raises(ValueError):
        ops.prepare_geometry(rgba.astype(np.float32))


@pytest.mark.parametrize("mode", ["all", "stroke"])
@pytest.mark.parametrize("on_white", [False, True])
@pytest.mark.parametrize("level", [0, 2])
def test_paint_drawing_equals_paint_image(eng, level, on_white, mode):
    g, rgba = eng["g"], eng["rgba"]
    m = int(g["crop_margin"])
    opts = painting.GanBrushOptions()
    opts.set_style(torch.from_numpy(eng["z"]), 594)
    res = []
    for route in ("host", "device"):
        helper = painting.PaintingHelper(eng["ops"], batch=4)
        helper.set_feature_blending(level)
        if route == "host":
            res.append(helper.paint_image(painting.prepare_geometry_image(rgba), opts, crop_margin=m, stitching_mode=mode,
                                          on_white=on_white, return_full=True))
        else:
            res.append(helper.paint_drawing(rgba, opts, crop_margin=m, stitching_mode=mode, on_white=on_white, return_full=True))
            single = helper.paint_drawing(rgba, opts, crop_margin=m, stitching_mode=mode, on_white=on_white)
    (out_h, full_h, crops_h, padded_h), (out_d, full_d, crops_d, padded_d) = res
    assert list(crops_d) == list(crops_h) and len(crops_h) > 0
    assert padded_d.shape == padded_h.shape and padded_d.dtype == padded_h.dtype and np.array_equal(padded_d, padded_h)
    assert np.array_equal(full_d, full_h)
    assert out_d.shape == rgba.shape[:2] + ((3,) if on_white else (4,)) and out_d.dtype == np.uint8
    assert np.array_equal(out_d, out_h) and np.array_equal(single, out_h)
    assert full_h[..., 3].max() > 0                                     # something was painted
    if mode == "stroke":
        assert np.array_equal(np.array([c[:2] for c in crops_d]),
                              np.array([c[:2] for c in painting.generate_stitching_crops(
                                  painting.pad_geo(painting.prepare_geometry_image(rgba), m), 128, "stroke", 2 * m)[0]]))


def test_paint_image_main_routes_write_the_same_file(eng, tmp_path):
    """paint_image_main on the decoded file: the device route (default) and --host_prepare write byte-identical PNGs."""
    from PIL import Image
    from brushstroke_engine_amd import formats, paint_image_main
    snap = str(tmp_path / "engine.npz")
    formats.save_engine_snapshot(snap, eng["cfg"], eng["sd"], eng["esd"], preproc_type=None)
    png = str(tmp_path / "drawing.png")
    Image.fromarray(eng["rgba"]).save(png)
    files = []
    for name, extra in (("dev", []), ("host", ["--host_prepare"])):
        files.append(paint_image_main.main(["--gan_checkpoint", snap, "--geom_image", png, "--output_file_prefix", str(tmp_path / name / "res"),
                                            "--style_id", "594", "--library", "594,12", "--feature_blending_level", "2", "--no_uvs_mapping",
                                            "--on_white", "--stitching_mode", "stroke"] + extra))
    a, b = (open(f, "rb").read() for f in files)
    assert a == b and np.array(Image.open(files[0])).shape == eng["rgba"].shape[:2] + (3,)
