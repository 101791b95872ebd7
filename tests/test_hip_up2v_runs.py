"""The up=2 epilogue of modconv3x3_up2v_kernel walks column runs of quads (3 or 4 per run; 12-row tiles 3 + 3 + 3 + 3, 13-row
tiles 4 + 3 + 3 + 3): every pre-filter row is filtered horizontally once and kept in a sliding window, every output row is one
vertical FIR over four window rows.  Here both tile heights are checked against a float64 evaluation of the layer, fp32 and
hand-off output, at the smallest shapes at which a run can go wrong, and a single-pixel / single-tap input is compared with the
4 x 4 FIR kernel itself on both sides of every run boundary (a window off by one row shows there unambiguously).

Bounds (tests/test_hip_f8.py, test_f8_kernels_vs_float64): |y - float64| <= 2e-6 (hi / lo f16 operands) or 4e-5 ("f8" operands)
x max |linear output|.  The linear output here is conv x dcoef x gain; noise, bias, lrelu and clamp follow it, all 1-Lipschitz, so
the same bound holds behind them.  Hand-off (test_f8_handoff_equals_pack): the consumer's operand decodes to value x next style
within the kernel bound x the largest style, plus what the format keeps: 2e-5 of the largest value for hi + fp8 residual, 2^-21
for hi + lo f16; the fp8(v / 4) plane within 0.07 of the largest value (one fp8 step)."""
import ctypes

import numpy as np
import pytest
import torch

from test_hip_f8 import _conv_ref

pytestmark = pytest.mark.gpu

ALPHA, GAIN, CLAMP = 0.2, 1.4142135, 3.0


def _setters(lib):
    for f in ("nb_debug_set_up2v_rows", "nb_debug_set_up2v_persistent", "nb_debug_set_up2_v2"):
        getattr(lib, f).argtypes, getattr(lib, f).restype = [ctypes.c_int], None


def _decode_f8(t, c):
    """f8-format tensor -> (hi + fp8 residual / 512, 4 x fp8(v / 4)) as fp32 [n, c, h, w]"""
    nn, c8, _, h, w_, _ = t.shape
    hi = t[:, :, 0].float().permute(0, 1, 4, 2, 3).reshape(nn, c8 * 8, h, w_)[:, :c]
    lo = t[:, :, 1].contiguous().view(torch.uint8).view(torch.float8_e4m3fn).float()      # [n, c8, h, w, 16]
    xl = lo[:, 0::2].permute(0, 1, 4, 2, 3).reshape(nn, c8 * 8, h, w_)[:, :c]
    xh = lo[:, 1::2].permute(0, 1, 4, 2, 3).reshape(nn, c8 * 8, h, w_)[:, :c]
    return hi + xl / 512, xh * 4


def _run(lib, rows, xh, ci, wp, dco, noise, bias, nst, fmt, out_fmt, n, h, w, co, alpha, gain, clamp):
    """fp32 and hand-off output of the up2v kernel on tiles of `rows` quad rows"""
    from brushstroke_engine_amd import _lib, ops
    S = torch.cuda.current_stream().cuda_stream
    lib.nb_debug_set_up2v_rows(rows)
    y = torch.full([n, co, 2 * h, 2 * w], float("nan"), device="cuda")
    out = torch.zeros(ops.h2_shape(n, co, 2 * h, 2 * w), dtype=torch.float16, device="cuda")
    common = (dco.data_ptr(), None if noise is None else noise.data_ptr(), 4 * h * w, bias.data_ptr())
    _lib.check(lib.nb_modconv3x3_up2_h3_ex(xh.data_ptr(), ci, wp.data_ptr(), *common, y.data_ptr(), None, None, 0, 0, fmt, 0,
                                           n, h, w, co, alpha, gain, clamp, S), "f32 out")
    _lib.check(lib.nb_modconv3x3_up2_h3_ex(xh.data_ptr(), ci, wp.data_ptr(), *common, None, out.data_ptr(), nst.data_ptr(), co,
                                           co, fmt, out_fmt, n, h, w, co, alpha, gain, clamp, S), "hand-off out")
    torch.cuda.synchronize()
    return y, out


@pytest.mark.parametrize("fmt,ci,co,h,w,n", [
    (1, 32, 32, 8, 32, 1),       # image shorter than a tile: the run is cut by the image edge
    (1, 32, 64, 14, 64, 3),      # h = 1 (mod 13): the last tile is one row high; two c_out slices
    (1, 48, 32, 25, 32, 2),      # h = 12 (mod 13) and 1 (mod 12): a ragged last tile in both forms
    (0, 32, 32, 26, 32, 2),      # hi / lo f16 operands
    (1, 32, 96, 13, 64, 5),      # exactly one full 13-row tile: every run boundary interior; three slices; batch no multiple of 8
])
def test_up2v_runs_vs_float64(fmt, ci, co, h, w, n):
    from brushstroke_engine_amd import _lib, ops
    rs = np.random.RandomState(100 * fmt + ci + co + h)
    x = torch.from_numpy(rs.randn(n, ci, h, w).astype(np.float32)).cuda()
    wt = torch.from_numpy((rs.randn(co, ci, 3, 3) / np.sqrt(9 * ci)).astype(np.float32)).cuda()
    st = torch.from_numpy(rs.uniform(0.5, 1.5, (n, ci)).astype(np.float32)).cuda()
    nst = torch.from_numpy(rs.uniform(0.5, 1.5, (n, co)).astype(np.float32)).cuda()
    dco = torch.from_numpy(rs.uniform(0.5, 1.5, (n, co)).astype(np.float32)).cuda()
    bias = torch.from_numpy((1.5 * rs.randn(co)).astype(np.float32)).cuda()
    noise = torch.from_numpy(rs.randn(n, 2 * h, 2 * w).astype(np.float32)).cuda()          # (varies along rows and columns)
    pack_x, pack_w = (ops.pack_h2f8, ops.pack_conv_weight_h3f8) if fmt else (ops.pack_h2, ops.pack_conv_weight_h3)
    xh, wp = pack_x(x, st), pack_w(wt)
    out_fmt = 1 if fmt else 0

    lin = _conv_ref(x, wt, st, 2) * dco.double().cpu()[:, :, None, None]
    scale = float(lin.abs().max()) * GAIN
    pre = (lin + noise.double().cpu()[:, None] + bias.double().cpu()[None, :, None, None]) * GAIN
    act = torch.where(pre >= 0, pre, ALPHA * pre)
    ref = act.clamp(-CLAMP, CLAMP)
    # the reference lies on both sides of the lrelu kink and of the clamp (else the case says nothing about the window's row order)
    assert bool((pre > 0).any()) and bool((pre < 0).any())
    assert bool((act.abs() > CLAMP).any()) and bool((act.abs() < CLAMP).any())
    want = ref * nst.double().cpu()[:, :, None, None]
    tol = (4e-5 if fmt else 2e-6) * scale
    tol_out = tol * float(nst.max()) + (2e-5 if fmt else 2.0 ** -21) * float(want.abs().max())

    lib = _lib.lib()
    _setters(lib)
    try:
        lib.nb_debug_set_up2_v2(1)
        for rows in (12, 13):
            y, out = _run(lib, rows, xh, ci, wp, dco, noise, bias, nst, fmt, out_fmt, n, h, w, co, ALPHA, GAIN, CLAMP)
            err = float((y.double().cpu() - ref).abs().max())
            if fmt:
                v, v4 = _decode_f8(out, co)
                err4 = float((v4.double().cpu() - want).abs().max())
            else:
                v, err4 = ops.unpack_h2(out, co), 0.0
            err_out = float((v.double().cpu() - want).abs().max())
            print(f"rows {rows}: fp32 err {err:.3e} (bound {tol:.3e}), hand-off err {err_out:.3e} (bound {tol_out:.3e}), "
                  f"fp8(v/4) err {err4:.3e} (bound {0.07 * float(want.abs().max()):.3e})")
            assert bool(torch.isfinite(y).all()), rows
            assert err <= tol, (rows, err, tol)
            assert err_out <= tol_out, (rows, err_out, tol_out)
            assert err4 <= 0.07 * float(want.abs().max()), (rows, err4)
    finally:
        lib.nb_debug_set_up2v_rows(0)
        lib.nb_debug_set_up2_v2(-1)


@pytest.mark.parametrize("fmt", [0, 1])
def test_up2v_single_pixel_is_the_fir_kernel(fmt):
    """x = one pixel of value 1 per sample, weights = one tap of value 1 (exact in every operand format), styles and dcoefs 1,
    no noise, bias, activation or clamp: the output is the 4 x 4 FIR kernel [1, 3, 3, 1] x [1, 3, 3, 1] / 16 (exact in fp32), at
    the place float64 puts it, and zero elsewhere.  Source pixels in tile rows 2 ... 10: both sides of the run boundaries 3, 6, 9
    (12-row tiles) and 4, 7, 10 (13-row tiles); columns at the tile's edges and inside."""
    from brushstroke_engine_amd import _lib, ops
    ci, co, h, w = 16, 32, 13, 32
    src_rows = list(range(2, 11))
    n = len(src_rows)
    x = torch.zeros(n, ci, h, w)
    cols = [0, 31, 7, 16, 30, 1, 15, 31, 0]
    for k, r in enumerate(src_rows):
        x[k, 3, r, cols[k]] = 1.0
    wt = torch.zeros(co, ci, 3, 3)
    wt[:, 3, 1, 1] = 1.0
    x, wt = x.cuda(), wt.cuda()
    ones = torch.ones(n, max(ci, co), device="cuda")
    st, dco, nst = ones[:, :ci].contiguous(), ones[:, :co].contiguous(), ones[:, :co].contiguous()
    bias = torch.zeros(co, device="cuda")
    pack_x, pack_w = (ops.pack_h2f8, ops.pack_conv_weight_h3f8) if fmt else (ops.pack_h2, ops.pack_conv_weight_h3)
    xh, wp = pack_x(x, st), pack_w(wt)
    ref = _conv_ref(x, wt, st, 2)
    fir = torch.tensor([1.0, 3.0, 3.0, 1.0], dtype=torch.float64)
    fir = torch.outer(fir, fir) / 16
    for k, r in enumerate(src_rows):                 # (the reference itself: the FIR kernel, cut at the image's edges, nothing else)
        nzr, nzc = torch.nonzero(ref[k, 0].sum(1))[:, 0], torch.nonzero(ref[k, 0].sum(0))[:, 0]
        patch = ref[k, 0, nzr[0]:nzr[-1] + 1, nzc[0]:nzc[-1] + 1]
        assert patch.shape[0] == 4 and float(ref[k, 0].sum()) == float(patch.sum())
        c0 = 1 if cols[k] == 0 else 0
        assert torch.equal(patch, fir[:, c0:c0 + patch.shape[1]]), (r, cols[k])
    lib = _lib.lib()
    _setters(lib)
    try:
        lib.nb_debug_set_up2_v2(1)
        for rows in (12, 13):
            y, out = _run(lib, rows, xh, ci, wp, dco, None, bias, nst, fmt, 1 if fmt else 0, n, h, w, co, 1.0, 1.0, -1.0)
            v = _decode_f8(out, co)[0] if fmt else ops.unpack_h2(out, co)
            for k, r in enumerate(src_rows):
                assert torch.equal(y[k].double().cpu(), ref[k]), (rows, "fp32", r)
                assert torch.equal(v[k].double().cpu(), ref[k]), (rows, "hand-off", r)
    finally:
        lib.nb_debug_set_up2v_rows(0)
        lib.nb_debug_set_up2_v2(-1)
