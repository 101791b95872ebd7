"""Vector strokes on the device (csrc/nb_strokes.hip) against the float64 restatements of tests/stroke_refs.py.

Acceptance rule of every raster comparison (``stroke_refs.check_raster``): the device bytes equal ``margin64 <= 0 ? 0 : 255`` at
every pixel with ``|margin64| >= 1e-3``, where margin64 = min over segments of (distance - r) in float64 on exactly the fp32 rows
the kernel read.  At most 0.2 % of an image's pixels may be excluded that way -- a condition on the scenes, which
tests/test_stroke_refs_cpu.py checks without a GPU -- and none for the exact scenes (integer end points, radii k + 0.5), which are
compared byte for byte."""
import numpy as np
import pytest
import torch

import stroke_refs as sr
from conftest import load_golden
from brushstroke_engine_amd import _lib, config as cfgmod, encoder as encmod, painting, weights as wmod

pytestmark = pytest.mark.gpu

GUARD = 64               # bytes of 77 on either side of every output buffer: nothing may be written there
PITCH = painting.SEG_PITCH


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _raster(segs, h, w, off=(0, 0), clear=1, prefill=None, lead=0, n=None):
    """nb_raster_segments_u8 through ctypes on a buffer that starts GUARD + lead bytes into its allocation -> [h, w] numpy.
    ``segs``: numpy [n, 8] float32 or a device tensor; ``prefill``: [h, w] uint8 the buffer holds before the call (77 if None)."""
    d = segs if torch.is_tensor(segs) else (_dev(segs) if len(segs) else torch.zeros([1, PITCH], dtype=torch.float32, device="cuda"))
    n = len(segs) if n is None else n
    buf = torch.full([GUARD + lead + h * w + GUARD], 77, dtype=torch.uint8, device="cuda")
    view = buf[GUARD + lead:GUARD + lead + h * w].view(h, w)
    if prefill is not None:
        view.copy_(_dev(prefill))
    _lib.check(_lib.lib().nb_raster_segments_u8(d.data_ptr(), n, buf.data_ptr() + GUARD + lead, h, w, off[0], off[1], clear, _stream()),
               "raster_segments")
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[:GUARD + lead] == 77).all() and (host[GUARD + lead + h * w:] == 77).all(), "wrote outside the buffer"
    return host[GUARD + lead:GUARD + lead + h * w].reshape(h, w)


def _expect(case):
    return np.where(sr.case_margin(case) <= 0, 0, 255).astype(np.uint8)


CASES = sr.raster_cases()
BY_NAME = {c[0]: c for c in CASES}


# ---------------------------------------------------------------------------------------------------------------------
# the rasteriser
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_raster_scene(case):
    name, segs, h, w, off, exact = case
    got = _raster(segs, h, w, off)
    assert set(np.unique(got)) <= {0, 255}
    m = sr.case_margin(case)
    band = np.abs(m) < sr.BAND
    assert band.mean() <= (0.0 if exact else sr.BAND_CAP)
    want = _expect(case)
    if exact:
        assert not band.any() and np.array_equal(got, want), np.argwhere(got != want)[:4]
    else:
        bad = (got != want) & ~band
        assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:4].tolist(), m[bad][:4].tolist())
    if name.startswith("exact") and h >= 63:
        assert 0 < (got == 0).sum() < h * w


@pytest.mark.parametrize("name", ["exact-63x65+7+13", "random-130x257+0+0", "exact-3x5+0+0", "exact-1x1+0+0"])
@pytest.mark.parametrize("lead", [1, 2, 3])
def test_raster_unaligned_output(name, lead):
    """`out` starts 1-3 bytes into an allocation and the widths are odd: rows start at every byte alignment, so dword and byte
    stores mix within a row; the result is that of the aligned buffer."""
    case = BY_NAME[name]
    _, segs, h, w, off, exact = case
    aligned = _raster(segs, h, w, off)
    assert np.array_equal(_raster(segs, h, w, off, lead=lead), aligned)
    pattern = np.array([77, 0, 255], np.uint8)[(np.arange(h)[:, None] + np.arange(w)[None, :]) % 3]
    got = _raster(segs, h, w, off, clear=0, prefill=pattern, lead=lead)
    assert np.array_equal(got, np.where(aligned == 0, 0, pattern))


def test_dead_rows_draw_nothing():
    dead = sr.dead_rows()
    assert (_raster(dead, 63, 65, (7, 13)) == 255).all()
    live = BY_NAME["random-63x65+7+13"][1]
    mixed = np.concatenate([dead[:7], live[:20], dead[7:], live[20:]])
    assert np.array_equal(_raster(mixed, 63, 65, (7, 13)), _raster(live, 63, 65, (7, 13)))
    pattern = np.full((63, 65), 9, np.uint8)
    assert np.array_equal(_raster(dead, 63, 65, (7, 13), clear=0, prefill=pattern), pattern)


@pytest.mark.parametrize("name", ["exact-130x257+7+13", "sparse-3000", "count-257"])
def test_clear_0_darkens_only_stroke_pixels(name):
    case = BY_NAME[name]
    _, segs, h, w, off, _ = case
    pattern = np.array([77, 0, 255], np.uint8)[(np.arange(h) // 2 % 3)][:, None].repeat(w, 1)          # stripes of 77 / 0 / 255
    got = _raster(segs, h, w, off, clear=0, prefill=pattern)
    m = sr.case_margin(case)
    stroke, clear_of, band = (m <= 0), (m > 0), np.abs(m) < sr.BAND
    assert (got[stroke & ~band] == 0).all()
    assert np.array_equal(got[clear_of & ~band], pattern[clear_of & ~band])                            # byte for byte as it was
    assert ((got[band] == 0) | (got[band] == pattern[band])).all()
    # the same pixels as the clearing call darkens
    assert np.array_equal(got == 0, (_raster(segs, h, w, off) == 0) | (pattern == 0))


def test_no_segments():
    assert (_raster(np.zeros((0, PITCH), np.float32), 130, 257) == 255).all()                           # clear = 1 fills
    lib = _lib.lib()
    out = torch.full([33, 35], 9, dtype=torch.uint8, device="cuda")
    assert lib.nb_raster_segments_u8(None, 0, out.data_ptr(), 33, 35, 0, 0, 1, _stream()) == 0          # a null list of no rows
    assert (out.cpu().numpy() == 255).all()
    out.fill_(9)
    assert lib.nb_raster_segments_u8(None, 0, out.data_ptr(), 33, 35, 0, 0, 0, _stream()) == 0
    assert lib.nb_raster_segments_u8(None, 3, out.data_ptr(), 33, 35, 0, 0, 1, _stream()) == _lib.NB_EINVAL
    assert lib.nb_raster_segments_u8(out.data_ptr(), 3, None, 33, 35, 0, 0, 1, _stream()) == _lib.NB_EINVAL
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 9).all()


def test_order_and_reruns():
    case = BY_NAME["sparse-3000"]
    _, segs, h, w, off, _ = case
    first = _raster(segs, h, w, off)
    assert np.array_equal(_raster(segs, h, w, off), first)                                              # run to run
    rs = np.random.RandomState(0)
    for _ in range(2):
        assert np.array_equal(_raster(segs[rs.permutation(len(segs))], h, w, off), first)               # a union: any order
    assert np.array_equal(_raster(segs[::-1].copy(), h, w, off), first)
    # a prefix of the rows through n_segs: the rows behind it are not read
    assert np.array_equal(_raster(segs, h, w, off, n=300), _raster(segs[:300].copy(), h, w, off))


# ---------------------------------------------------------------------------------------------------------------------
# the flattener
# ---------------------------------------------------------------------------------------------------------------------
def _flatten(ctrl, off, subdiv, alpha=0.5, spare=5):
    """nb_spline_flatten_f32 into a NaN-filled buffer with `spare` rows more than needed -> numpy [count + spare, 8]."""
    n = sr.segment_count(off, subdiv)
    segs = torch.full([n + spare, PITCH], float("nan"), dtype=torch.float32, device="cuda")
    d_ctrl, d_off = _dev(ctrl), _dev(off)
    _lib.check(_lib.lib().nb_spline_flatten_f32(d_ctrl.data_ptr(), d_off.data_ptr(), ctrl.shape[0], len(off) - 1, subdiv, alpha,
                                                segs.data_ptr(), n + spare, _stream()), "spline_flatten")
    torch.cuda.synchronize()
    return segs


@pytest.mark.parametrize("n_strokes,subdiv", [(1, 1), (2, 8), (5, 8), (5, 1)])
def test_flatten_against_float64(n_strokes, subdiv):
    """Bound: 4 x the error a numpy float32 evaluation of the same pyramid shows against float64 on the same fp32 inputs (measured
    here, on the CPU side); the factor covers operation order, the device's powf and contraction differences."""
    ctrl, off = sr.spline_scene(n_strokes, seed=7 + n_strokes)
    n = sr.segment_count(off, subdiv)
    d_segs = _flatten(ctrl, off, subdiv)
    got = d_segs.cpu().numpy()
    assert np.isnan(got[n:]).all(), "rows past the count were written"
    got = got[:n]
    assert np.isfinite(got).all() and (got[:, 5:] == 0).all()
    want = sr.flatten(ctrl, off, subdiv)
    f32 = sr.flatten(ctrl, off, subdiv, dtype=np.float32)
    assert f32.dtype == np.float32 and want.dtype == np.float64
    bound_xy = 4 * float(np.abs(f32[:, :4].astype(np.float64) - want[:, :4]).max())
    # radii < 4: three fp32 roundings (difference, product, sum) of at most half an ulp of 4 = 2^-23 each
    bound_r = 3 * 2.0 ** -23
    err_xy, err_r = float(np.abs(got[:, :4] - want[:, :4]).max()), float(np.abs(got[:, 4] - want[:, 4]).max())
    print(f"strokes {n_strokes} subdiv {subdiv}: device {err_xy:.3e} (bound {bound_xy:.3e}), radius {err_r:.3e} (bound {bound_r:.3e})")
    assert 0 < bound_xy < 1e-3 and err_xy <= bound_xy
    assert ctrl[:, 2].max() < 4 and err_r <= bound_r
    for s in range(n_strokes):                                                   # watertight inside a stroke, bit for bit
        r0, r1 = (int(off[s]) - 3 * s) * subdiv, (int(off[s + 1]) - 3 * (s + 1)) * subdiv
        assert np.array_equal(got[r0 + 1:r1, :2].view(np.uint32), got[r0:r1 - 1, 2:4].view(np.uint32))
        if s:
            assert not np.array_equal(got[r0, :2], got[r0 - 1, 2:4])             # ... and strokes are apart
    # the raster of the device's own rows: flatten rounding does not leak into the raster check
    sr.check_raster(_raster(d_segs, 130, 130, (3, 2), n=n), got, (3, 2))


def test_flatten_repeated_control_point_draws_nothing():
    good, off_g = sr.spline_scene(1, seed=3)
    dup = np.array([[10, 10, 2], [40, 20, 2], [40, 20, 2], [70, 60, 2], [90, 90, 2]], np.float32)
    ctrl = np.concatenate([dup, good])
    off = np.array([0, 5, 5 + len(good)], np.int32)
    d_segs = _flatten(ctrl, off, 4, spare=0)
    got = d_segs.cpu().numpy()
    assert not np.isfinite(got[:8, :4]).any()                                    # both spans of the first stroke touch the zero interval
    assert np.isfinite(got[8:]).all()
    alone = _flatten(good, off_g, 4, spare=0)
    assert np.array_equal(got[8:].view(np.uint32), alone.cpu().numpy().view(np.uint32))
    assert (_raster(d_segs, 100, 100, n=8) == 255).all()
    assert np.array_equal(_raster(d_segs, 130, 130), _raster(alone, 130, 130))


def test_flatten_and_raster_graph_replay():
    """Both entries captured into one hipGraph (enqueue-only: no allocation, synchronisation or read-back inside) == the eager calls."""
    lib = _lib.lib()
    (c1, off), (c2, _) = sr.spline_scene(2, seed=9), sr.spline_scene(2, seed=10)
    n = sr.segment_count(off, 8)
    d_ctrl, d_off = _dev(c1), _dev(off)
    segs = torch.zeros([n, PITCH], dtype=torch.float32, device="cuda")
    out = torch.zeros([130, 129], dtype=torch.uint8, device="cuda")

    def enqueue(stream):
        _lib.check(lib.nb_spline_flatten_f32(d_ctrl.data_ptr(), d_off.data_ptr(), c1.shape[0], 2, 8, 0.5, segs.data_ptr(), n, stream), "flatten")
        _lib.check(lib.nb_raster_segments_u8(segs.data_ptr(), n, out.data_ptr(), 130, 129, 2, 1, 1, stream), "raster")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                    # load the code objects before the capture
        enqueue(side.cuda_stream)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        enqueue(_stream())
    for ctrl in (c2, c1):
        d_ctrl.copy_(_dev(ctrl))
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        eager = _flatten(ctrl, off, 8, spare=0)
        assert np.array_equal(segs.cpu().numpy().view(np.uint32), eager.cpu().numpy().view(np.uint32))
        assert np.array_equal(out.cpu().numpy(), _raster(eager, 130, 129, (2, 1)))
        assert (out.cpu().numpy() == 0).any()


# ---------------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    """The engine_r128 job with its seeded network, as tests/test_hip_geomprep.py sets it up."""
    g = load_golden("engine_r128.npz")
    cfg = cfgmod.style1_config(128)
    sd = wmod.random_state_dict(cfg, seed=0)
    esd = encmod.random_encoder_state_dict(5)
    z = np.random.RandomState(594).randn(1, cfg.z_dim)
    from brushstroke_engine_amd.networks import Generator
    G = Generator(cfg, sd, conv_mode="h3").to("cuda")
    ops = painting.TileOps(G, encmod.HipGeometryEncoder(esd))
    return dict(ops=ops, z=z, cfg=cfg, sd=sd, esd=esd, m=int(g["crop_margin"]), strokes=sr.e2e_strokes())


def test_tileops_raster_strokes(eng):
    ops, strokes = eng["ops"], eng["strokes"]
    h, w = sr.E2E_SIZE
    segs = ops.stroke_segments(strokes, 8)
    n_poly = strokes.polyline_segments().shape[0]
    assert segs.shape == (n_poly + strokes.spline_segment_count(8), PITCH) and n_poly == 4
    rows = segs.cpu().numpy()
    assert np.array_equal(rows[:n_poly], strokes.polyline_segments())
    ctrl, off = strokes.spline_control()
    assert np.abs(rows[n_poly:, :5] - sr.flatten(ctrl, off, 8)).max() < 1e-3
    geom = ops.raster_strokes(strokes, (h + 20, w + 20), (10, 10))
    assert geom.dtype == torch.uint8 and geom.shape == (h + 20, w + 20)
    sr.check_raster(geom.cpu().numpy(), rows, (10, 10))
    assert np.array_equal(ops.stroke_segments(strokes, 8).cpu().numpy().view(np.uint32), rows.view(np.uint32))      # run to run
    # more strokes on a prepared geometry: out= darkens, everything else stays
    more = painting.StrokeList().add_polyline([[5.5, 200.25], [190.5, 210.75]], 3.2)
    both = ops.raster_strokes(more, offset=(10, 10), out=geom.clone())
    alone = ops.raster_strokes(more, (h + 20, w + 20), (10, 10))
    assert torch.equal(both, torch.minimum(geom, alone)) and not torch.equal(both, geom)
    assert (ops.raster_strokes(painting.StrokeList(), (40, 50)) == 255).all()
    with pytest.raises(ValueError):
        ops.raster_strokes(more, out=geom.to(torch.float32))


@pytest.mark.parametrize("level,mode,on_white", [(0, "all", False), (2, "all", False), (2, "stroke", True)])
def test_paint_strokes_equals_paint_image(eng, level, mode, on_white):
    ops, strokes, m = eng["ops"], eng["strokes"], eng["m"]
    h0, w0 = sr.E2E_SIZE
    opts = painting.GanBrushOptions()
    opts.set_style(torch.from_numpy(eng["z"]), 594)
    helper = painting.PaintingHelper(ops, batch=4)
    helper.set_feature_blending(level)
    out_s, full_s, crops_s, padded_s = helper.paint_strokes(strokes, (h0, w0), opts, crop_margin=m, stitching_mode=mode, on_white=on_white,
                                                            return_full=True)
    single = helper.paint_strokes(strokes, (h0, w0), opts, crop_margin=m, stitching_mode=mode, on_white=on_white)
    # the padded geometry: the strokes inside the drawing's window, background around it
    assert padded_s.dtype == np.uint8 and padded_s.ndim == 3 and padded_s.shape[2] == 1
    geom = padded_s[m:m + h0, m:m + w0, 0]
    outside = padded_s[..., 0].copy()
    outside[m:m + h0, m:m + w0] = 255
    assert (outside == 255).all()
    rows = ops.stroke_segments(strokes, 8).cpu().numpy()
    sr.check_raster(geom, rows)
    assert (geom[:, 0] == 0).any()                                      # the polyline that leaves the drawing is cut at its edge
    # paint_image on that geometry: the same canvas, image and tiles
    helper2 = painting.PaintingHelper(ops, batch=4)
    helper2.set_feature_blending(level)
    out_i, full_i, crops_i, padded_i = helper2.paint_image(np.ascontiguousarray(geom)[..., None], opts, crop_margin=m, stitching_mode=mode,
                                                           on_white=on_white, return_full=True)
    assert list(crops_s) == list(crops_i) and len(crops_i) > 0
    assert np.array_equal(padded_s, padded_i)
    assert np.array_equal(full_s, full_i) and np.array_equal(out_s, out_i) and np.array_equal(single, out_i)
    assert out_s.shape == (h0, w0, 3 if on_white else 4) and out_s.dtype == np.uint8
    assert full_s[..., 3].max() > 0                                     # something was painted


def test_paint_image_main_strokes_route(eng, tmp_path):
    """``--strokes`` writes the PNG bytes that saving paint_strokes' result gives."""
    from PIL import Image
    from brushstroke_engine_amd import formats, paint_image_main
    snap = str(tmp_path / "engine.npz")
    formats.save_engine_snapshot(snap, eng["cfg"], eng["sd"], eng["esd"], preproc_type=None)
    js = tmp_path / "strokes.json"
    js.write_text(eng["strokes"].to_json())
    h0, w0 = sr.E2E_SIZE
    written = paint_image_main.main(["--gan_checkpoint", snap, "--strokes", str(js), "--canvas_size", f"{h0},{w0}", "--output_file_prefix",
                                     str(tmp_path / "cli" / "res"), "--style_id", "594", "--library", "594,12", "--feature_blending_level", "2",
                                     "--no_uvs_mapping", "--on_white", "--stitching_mode", "stroke", "--conv_mode", "h3", "--batch", "4"])
    opts = painting.GanBrushOptions()
    opts.set_style(torch.from_numpy(eng["z"]), 594)
    helper = painting.PaintingHelper(eng["ops"], batch=4)
    helper.set_feature_blending(2)
    result = helper.paint_strokes(painting.StrokeList.from_json(js.read_text()), (h0, w0), opts, crop_margin=10, stitching_mode="stroke",
                                  on_white=True)
    mine = str(tmp_path / "mine.png")
    Image.fromarray(result).save(mine)
    assert open(written, "rb").read() == open(mine, "rb").read()
    assert np.array(Image.open(written)).shape == (h0, w0, 3) and (np.array(Image.open(written)) < 255).any()
