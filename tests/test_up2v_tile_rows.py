"""The software-pipelined up=2 kernel (modconv3x3_up2v_kernel) runs 12- or 13-row tiles, chosen per launch shape.  Both heights
walk the same per-output arithmetic, so fp32 and hand-off outputs must be bit-identical between them -- on heights H = 0, 1 and 12
(mod 13), batches that are no multiple of 8, one to four c_out slices and every operand format.  (13-row launches always run one
workgroup per tile; the persistent 12-row form is compared with its one-workgroup-per-tile form in tests/test_hip_f8.py.)"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _setters(lib):
    for f in ("nb_debug_set_up2v_rows", "nb_debug_set_up2v_persistent", "nb_debug_set_up2_v2"):
        getattr(lib, f).argtypes, getattr(lib, f).restype = [ctypes.c_int], None
    lib.nb_debug_up2v_auto_rows.argtypes, lib.nb_debug_up2v_auto_rows.restype = [ctypes.c_int] * 5, ctypes.c_int


@pytest.mark.parametrize("fmt,ci,co,h,w,n", [(1, 128, 64, 26, 64, 3), (1, 384, 128, 64, 64, 5), (1, 64, 96, 25, 32, 7),
                                             (0, 48, 32, 27, 32, 3), (2, 64, 64, 39, 32, 2), (3, 32, 128, 14, 64, 9),
                                             (1, 32, 32, 8, 32, 1)])
def test_up2v_13_rows_equal_12_rows(fmt, ci, co, h, w, n):
    from brushstroke_engine_amd import _lib, ops
    rs = np.random.RandomState(ci + h + fmt)
    x = torch.from_numpy(rs.randn(n, ci, h, w).astype(np.float32)).cuda()
    wt = torch.from_numpy((rs.randn(co, ci, 3, 3) / np.sqrt(9 * ci)).astype(np.float32)).cuda()
    st = torch.from_numpy(rs.uniform(0.5, 1.5, (n, ci)).astype(np.float32)).cuda()
    nst = torch.from_numpy(rs.uniform(0.5, 1.5, (n, co)).astype(np.float32)).cuda()
    dco = torch.from_numpy(rs.uniform(0.5, 1.5, (n, co)).astype(np.float32)).cuda()
    bias = torch.from_numpy(rs.randn(co).astype(np.float32)).cuda()
    noise = torch.from_numpy(rs.randn(n, 2 * h, 2 * w).astype(np.float32)).cuda()
    pack_x, pack_w = {0: (ops.pack_h2, ops.pack_conv_weight_h3), 2: (ops.pack_h2f6, ops.pack_conv_weight_h3f6)}.get(
        fmt, (ops.pack_h2f8, ops.pack_conv_weight_h3f8))
    xh, wp = pack_x(x, st), pack_w(wt)
    del x
    out_fmt = 0 if fmt == 0 else 1
    lib, S = _lib.lib(), torch.cuda.current_stream().cuda_stream
    _setters(lib)
    res = {}
    try:
        lib.nb_debug_set_up2_v2(1)
        for rows, persist in ((12, 0), (13, -1), (13, 1)):          # (13 rows ignore the persistent switch)
            lib.nb_debug_set_up2v_rows(rows)
            lib.nb_debug_set_up2v_persistent(persist)
            y = torch.full([n, co, 2 * h, 2 * w], float("nan"), device="cuda")
            out = torch.zeros(ops.h2_shape(n, co, 2 * h, 2 * w), dtype=torch.float16, device="cuda")
            common = (dco.data_ptr(), noise.data_ptr(), 4 * h * w, bias.data_ptr())
            _lib.check(lib.nb_modconv3x3_up2_h3_ex(xh.data_ptr(), ci, wp.data_ptr(), *common, y.data_ptr(), None, None, 0, 0, fmt, 0,
                                                   n, h, w, co, 0.2, 1.4142135, 256.0, S), "f32 out")
            _lib.check(lib.nb_modconv3x3_up2_h3_ex(xh.data_ptr(), ci, wp.data_ptr(), *common, None, out.data_ptr(), nst.data_ptr(), co,
                                                   co, fmt, out_fmt, n, h, w, co, 0.2, 1.4142135, 256.0, S), "hand-off out")
            torch.cuda.synchronize()
            res[(rows, persist)] = (y, out)
    finally:
        lib.nb_debug_set_up2v_rows(0)
        lib.nb_debug_set_up2v_persistent(-1)
        lib.nb_debug_set_up2_v2(-1)
    y12, out12 = res[(12, 0)]
    assert bool(torch.isfinite(y12).all())
    for key in ((13, -1), (13, 1)):
        assert torch.equal(y12, res[key][0]), key
        assert torch.equal(out12, res[key][1]), key


def test_up2v_rows_hook_default_is_automatic():
    """The automatic choice (hook value 0) renders what the forced 12 rows render, at a shape where it takes 13 rows."""
    from brushstroke_engine_amd import _lib, ops
    rs = np.random.RandomState(7)
    n, ci, co, h, w = 32, 384, 128, 64, 64                     # BASELINE's 384->128@128 layer
    x = torch.from_numpy(rs.randn(n, ci, h, w).astype(np.float32)).cuda()
    wt = torch.from_numpy((rs.randn(co, ci, 3, 3) / np.sqrt(9 * ci)).astype(np.float32)).cuda()
    st = torch.ones(n, ci, device="cuda")
    nst = torch.from_numpy(rs.uniform(0.5, 1.5, (n, co)).astype(np.float32)).cuda()
    dco, bias = torch.ones(n, co, device="cuda"), torch.zeros(co, device="cuda")
    xh, wp = ops.pack_h2f8(x, st), ops.pack_conv_weight_h3f8(wt)
    del x
    lib, S = _lib.lib(), torch.cuda.current_stream().cuda_stream
    _setters(lib)
    assert lib.nb_debug_up2v_auto_rows(ci, co, n, h, w) == 13
    outs = []
    try:
        for rows in (0, 12):
            lib.nb_debug_set_up2v_rows(rows)
            out = torch.zeros(ops.h2_shape(n, co, 2 * h, 2 * w), dtype=torch.float16, device="cuda")
            _lib.check(lib.nb_modconv3x3_up2_h3_ex(xh.data_ptr(), ci, wp.data_ptr(), dco.data_ptr(), None, 0, bias.data_ptr(), None,
                                                   out.data_ptr(), nst.data_ptr(), co, co, 1, 1, n, h, w, co, 0.2, 1.4142135, 256.0, S),
                       "hand-off out")
            torch.cuda.synchronize()
            outs.append(out)
    finally:
        lib.nb_debug_set_up2v_rows(0)
    assert torch.equal(outs[0], outs[1])
