"""Synthetic drawings on the device (csrc/nb_drawings.hip) against the float64 restatements of ``brushstroke_engine_amd.drawings``
and tests/stroke_refs.py.

The sampler: radii and cells are exact against ``synth_ctrl_numpy`` (the seeds keep every thickness try clear of a rounding
boundary, tests/test_drawings_cpu.py), coordinates within NB_SYNTH_COORD_ROUNDINGS * ulp(1.1 r): the fp32 roundings counted in the
header comment of the kernel file.  The batch raster, per case: byte equality with K calls of nb_raster_segments_u8 on the same rows,
and ``stroke_refs.check_raster`` against float64 on the fp32 rows the kernel read (``BAND``, ``BAND_CAP`` as they stand)."""
import ctypes
import json

import numpy as np
import pytest
import torch

import drawing_refs as R
import stroke_refs as sr
from brushstroke_engine_amd import _lib, brush_metrics_main, config as cfgmod, drawings as dr, encoder as encmod, formats, painting, weights as wmod

pytestmark = pytest.mark.gpu

GUARD = 64               # bytes of 77 on either side of every output buffer: nothing may be written there
PITCH = painting.SEG_PITCH
SENTINEL = np.frombuffer(bytes([77] * 4), np.float32)[0]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---------------------------------------------------------------------------------------------------------------------
# the sampler
# ---------------------------------------------------------------------------------------------------------------------
def _ctrl(spec, seed, offset, k, r, off, n_points):
    """nb_synth_spline_ctrl_f32 through ctypes into a buffer of 77-bytes with guards -> [n_points, 3] float32."""
    buf = torch.full([GUARD + n_points * 12 + GUARD], 77, dtype=torch.uint8, device="cuda")
    c = spec.to_c()
    _lib.check(_lib.lib().nb_synth_spline_ctrl_f32(ctypes.addressof(c), seed, offset, k, r, _dev(np.asarray(off, np.int32)).data_ptr(),
                                                   buf.data_ptr() + GUARD, n_points, _stream()), "synth_spline_ctrl")
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[:GUARD] == 77).all() and (host[GUARD + n_points * 12:] == 77).all(), "wrote outside ctrl"
    return host[GUARD:GUARD + n_points * 12].view(np.float32).reshape(n_points, 3)


@pytest.mark.parametrize("name", list(R.ctrl_specs(64)))
@pytest.mark.parametrize("r", R.CTRL_SIDES)
def test_control_points(r, name):
    spec, seed, k = R.ctrl_specs(r)[name], R.CTRL_SEEDS[r], R.CTRL_K
    want, off = dr.synth_ctrl_numpy(spec, seed, R.CTRL_OFFSET, k, r)
    n = int(off[-1])
    got = _ctrl(spec, seed, R.CTRL_OFFSET, k, r, off, n)
    assert np.array_equal(got[:, 2].astype(np.float64), want[:, 2])                         # radii: exact
    err = np.abs(got[:, :2].astype(np.float64) - want[:, :2]).max()
    print(f"{name} r={r}: max coordinate error {err:.3e}, bound {R.coord_bound(r):.3e}")
    assert err <= R.coord_bound(r)
    if spec.mode == "cells":
        for d in range(k):
            a, b = int(off[d]), min(int(off[d + 1]), int(off[d]) + 16)
            assert np.array_equal(R.cells_of(got[a:b].astype(np.float64), r), R.cells_of(want[a:b], r)), d
    if spec.thick == "mixture":
        assert len(set(got[:, 2].tolist())) > 3
    # drawing k at offset o is drawing 0 at offset o + k
    j = 9
    one = _ctrl(spec, seed, R.CTRL_OFFSET + j, 1, r, [0, off[j + 1] - off[j]], int(off[j + 1] - off[j]))
    assert np.array_equal(one.view(np.uint32), got[off[j]:off[j + 1]].view(np.uint32))
    # a stroke_off with one wrong entry: the two drawings it bounds are skipped, every other row is written as before
    j = 20
    wrong = off.copy()
    wrong[j] += 1
    part = _ctrl(spec, seed, R.CTRL_OFFSET, k, r, wrong, n)
    skipped = np.zeros(n, bool)
    skipped[off[j - 1]:off[j + 1]] = True
    assert (part[skipped].view(np.uint32) == SENTINEL.view(np.uint32)).all()
    assert np.array_equal(part[~skipped].view(np.uint32), got[~skipped].view(np.uint32))
    # an entry past the total: the last drawing is skipped and nothing behind ctrl is written (the guard check of _ctrl)
    wrong = off.copy()
    wrong[-1] += 2
    part = _ctrl(spec, seed, R.CTRL_OFFSET, k, r, wrong, n)
    assert (part[off[-2]:].view(np.uint32) == SENTINEL.view(np.uint32)).all()
    assert np.array_equal(part[:off[-2]].view(np.uint32), got[:off[-2]].view(np.uint32))


def test_control_entry_validates():
    lib = _lib.lib()
    good = dr.SplineSpec().to_c()
    off, ctrl = _dev(np.array([0, 4], np.int32)), torch.full([12], 7.0, device="cuda")
    for args in ((0, 64, 4), (1, 0, 4), (1, 64, 3), (1, 64, 16)):                             # k, r, n_points_total
        assert lib.nb_synth_spline_ctrl_f32(ctypes.addressof(good), 1, 0, args[0], args[1], off.data_ptr(), ctrl.data_ptr(), args[2],
                                            _stream()) == _lib.NB_EINVAL, args
    torch.cuda.synchronize()
    assert (ctrl == 7).all()


# ---------------------------------------------------------------------------------------------------------------------
# the batch raster
# ---------------------------------------------------------------------------------------------------------------------
def _guarded(n, lead=0):
    buf = torch.full([GUARD + lead + n + GUARD], 77, dtype=torch.uint8, device="cuda")
    return buf, buf.data_ptr() + GUARD + lead


def _read(buf, n, lead=0):
    host = buf.cpu().numpy()
    assert (host[:GUARD + lead] == 77).all() and (host[GUARD + lead + n:] == 77).all(), "wrote outside the buffer"
    return host[GUARD + lead:GUARD + lead + n]


CASES = R.batch_cases()


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_raster_batch(case):
    lib = _lib.lib()
    k, h, w, off, lead = case["k"], case["h"], case["w"], case["off"], case["lead"]
    segs, seg_off = _dev(case["segs"]), _dev(case["seg_off"])
    buf, ptr = _guarded(k * h * w, lead)
    _lib.check(lib.nb_raster_batch_u8(segs.data_ptr(), seg_off.data_ptr(), segs.shape[0], k, ptr, h, w, off[0], off[1], _stream()), "raster_batch")
    torch.cuda.synchronize()
    got = _read(buf, k * h * w, lead).reshape(k, h, w)
    assert set(np.unique(got)) <= {0, 255}
    for i in range(k):
        rows = R.drawing_rows(case, i)
        # (1) the bytes of nb_raster_segments_u8 on the same device rows
        one, p1 = _guarded(h * w)
        a = int(case["seg_off"][i]) if len(rows) else 0
        _lib.check(lib.nb_raster_segments_u8(segs.data_ptr() + a * PITCH * 4 if len(rows) else None, len(rows), p1, h, w, off[0], off[1], 1,
                                             _stream()), "raster_segments")
        torch.cuda.synchronize()
        assert np.array_equal(got[i], _read(one, h * w).reshape(h, w)), i
        # (2) float64 on the rows the kernel read
        sr.check_raster(got[i], rows, off, exact=case["exact"])
        if not len(rows) or not sr.valid_rows(rows).any():
            assert (got[i] == 255).all(), i
    if case["name"] == "k2-clipping":
        assert (got[1] == 255).all() and (got[0][-1] == 0).any() and (got[0][:, -1] == 0).any()
    if case["exact"]:
        assert np.array_equal(got[0], got[1]) and 0 < (got[0] == 0).sum() < h * w


def test_raster_batch_entry_validates():
    lib = _lib.lib()
    segs, seg_off = torch.zeros([4, PITCH], device="cuda"), _dev(np.array([0, 4], np.int32))
    out = torch.full([16, 16], 9, dtype=torch.uint8, device="cuda")
    s, o, d = segs.data_ptr(), seg_off.data_ptr(), out.data_ptr()
    for args in ((s, None, 4, 1, d, 16, 16), (s, o, 4, 1, None, 16, 16), (None, o, 4, 1, d, 16, 16), (s, o, -1, 1, d, 16, 16), (s, o, 4, 0, d, 16, 16),
                 (s, o, 4, 1, d, 0, 16), (s, o, 4, 1, d, 16, 0), (s + 4, o, 3, 1, d, 16, 16), (s, o, 4, 1, d, 1 << 16, 1 << 15)):
        assert lib.nb_raster_batch_u8(*args, 0, 0, _stream()) == _lib.NB_EINVAL, args
    torch.cuda.synchronize()
    assert (out == 9).all()
    # no rows at all: a null list is legal and every drawing is cleared
    assert lib.nb_raster_batch_u8(None, _dev(np.zeros(2, np.int32)).data_ptr(), 0, 1, d, 16, 16, 0, 0, _stream()) == 0
    assert (out.cpu().numpy() == 255).all()


# ---------------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    """The R = 128 engine of tests/test_hip_brush_metrics.py with its seeded network."""
    cfg = cfgmod.style1_config(128)
    sd = wmod.random_state_dict(cfg, seed=0)
    esd = encmod.random_encoder_state_dict(5)
    from brushstroke_engine_amd.networks import Generator
    ops = painting.TileOps(Generator(cfg, sd, conv_mode="h3").to("cuda"), encmod.HipGeometryEncoder(esd))
    return dict(cfg=cfg, sd=sd, esd=esd, ops=ops)


def test_synth_batch_end_to_end(eng):
    r, k = R.E2E_R, R.E2E_K
    synth = dr.SplineSynth(R.e2e_spec(), r, R.E2E_SEED, "cuda")
    whole = synth.batch(k)
    assert whole.shape == (k, r, r) and whole.dtype == torch.uint8 and whole.is_cuda
    assert torch.equal(whole, torch.cat([synth.batch(3), synth.batch(5, offset=3)]))          # any batch size
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = synth.batch(k)
    side.synchronize()
    assert torch.equal(other, whole)
    got = whole.cpu().numpy()
    segs, seg_off = synth.segments(k)
    rows = segs.cpu().numpy()
    ctrl, off = synth.control(k)
    want, off64 = dr.synth_ctrl_numpy(synth.spec, R.E2E_SEED, 0, k, r)
    assert np.array_equal(off, off64) and np.abs(ctrl.cpu().numpy() - want).max() <= R.coord_bound(r)
    ops = eng["ops"]
    lists = [synth.strokes(i) for i in range(k)]
    for i in range(k):
        sr.check_raster(got[i], rows[seg_off[i]:seg_off[i + 1]], (0, 0))                      # float64 on the device's own rows
        assert 0 < (got[i] == 0).sum() < r * r
        assert torch.equal(ops.raster_strokes(lists[i], (r, r)), whole[i]), i                  # the same drawing as vector strokes
    assert torch.equal(ops.raster_strokes_batch(lists, (r, r)), whole)
    # stroke lists with polylines, another size and an offset: each drawing as raster_strokes gives it alone
    mixed = [sr.e2e_strokes(), lists[0], painting.StrokeList(), painting.StrokeList().add_polyline([[5.5, 20.25], [60.5, 41.75]], 3.2)]
    both = ops.raster_strokes_batch(mixed, (70, 130), (3, -5))
    for i, s in enumerate(mixed):
        assert torch.equal(both[i], ops.raster_strokes(s, (70, 130), (3, -5))), i
    # the CPU route draws the same picture up to the band
    cpu = dr.SplineSynth(R.e2e_spec(), r, R.E2E_SEED).batch(k).numpy()
    assert (cpu != got).mean() <= sr.BAND_CAP


def test_metrics_tool_on_synthetic_drawings(eng, tmp_path):
    snap = str(tmp_path / "engine.npz")
    formats.save_engine_snapshot(snap, eng["cfg"], eng["sd"], eng["esd"], preproc_type=None)
    out = tmp_path / "scores"
    style, summary, info = brush_metrics_main.main(["--gan_checkpoint", snap, "--library", "594,0", "--drawings", "synth:4:1", "--uvs_calibration",
                                                    "synth:2", "--output_dir", str(out), "--conv_mode", "h3", "--batch", "8"])
    rows = open(style).read().splitlines()
    assert [row.split()[0] for row in rows[1:]] == ["0", "594"] and len(open(summary).read().splitlines()) == 2
    back = json.load(open(info))
    assert back["ids"] == ["0", "594"]
    assert np.isfinite(np.array(back["metrics"]["BG_CLARITY_MEAN"], np.float64)).all()
    assert np.isfinite(np.array(back["metrics"]["FG_OPACITY_MEDIAN"], np.float64)).all()
