"""GPU: the kernels of the training path's split-f16 convolutions and of modulated_conv2d's backward tail (csrc/nb_grad.hip,
csrc/nb_encoder.hip), each through its C entry point on tensors built here, against float64 on the CPU.

Every output lies inside a NaN-filled buffer with guards (tests/test_hip_step_kernels.py): guards must stay NaN.

Tolerances: U = 2^-24.  A contraction of L fp32 terms is within (L + k) U S of the exact sum, S = the float64 sum of |terms| of
that output (the same contraction on |operands|).  The split-f16 products x y ~= xh yh + xh yl + xl yh lose the dropped xl yl
(<= 2^-22 |x y|) and the roundings of the two lo halves (<= 2^-22 |x| |y| each while the lo halves are normal f16): 12 U per
product.  A lo half below the f16 normal range is rounded to the subnormal step 2^-24 of the operand's range-scaled units:
an absolute error of 2^-24 / scale per element (taken as a full step), so the bound adds 2^-24 (sum|y| / sx + sum|x| / sy).
Each case also shows that its bound can catch an error: zeroing one input channel in the float64 reference must move some
output by at least 20x the largest bound."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from brushstroke_engine_amd import _lib, ops
from test_hip_step_kernels import Out, P, U, stream, within

pytestmark = pytest.mark.gpu
SUB = 2.0 ** -24                    # f16 subnormal step (in range-scaled units)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


def catches(want, want_bad, tol, what):
    """The bound is tight enough to see a lost input channel: max|want - want_bad| >= 20 max(tol)."""
    moved = float((want - want_bad).abs().max())
    t = float(tol.max()) if torch.is_tensor(tol) else float(tol)
    assert moved >= 20 * t, f"{what}: a zeroed input channel moves the output by {moved:.3g}, bound {t:.3g}: the check is blind"


def pow2_scale(target, mx):
    """nb_pow2_scale: the power of two that brings max-abs mx near target (clamped to 2^+-100)."""
    e = math.floor(math.log2(target / max(mx, 1e-30)))
    return 2.0 ** min(max(e, -100), 100)


def absmax_slots(dev, a, b=None, c=None):
    slots = torch.zeros([4], dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().nb_absmax_f32(P(a), a.numel(), P(b), 0 if b is None else b.numel(), P(c), 0 if c is None else c.numel(),
                                        P(slots), stream()), "absmax")
    return slots


# ---------------------------------------------------------------------------------------------------------------------
# nb_conv2d_wgrad_h3_ws
# ---------------------------------------------------------------------------------------------------------------------

def wgrad_ref(u, v, st, pad):
    """A[n,cu,cv,3,3] = sum_{i,j} u[n,cu,i st+a-pad,j st+b-pad] v[n,cv,i,j] in float64 (zeros outside u)."""
    n, cu, hu, wu = u.shape
    hv, wv = v.shape[2], v.shape[3]
    rh, rw = max(0, (hv - 1) * st + 3 - hu - pad), max(0, (wv - 1) * st + 3 - wu - pad)
    up = F.pad(u, (pad, rw, pad, rh))
    a = torch.empty([n, cu, v.shape[1], 3, 3], dtype=torch.float64)
    for ka in range(3):
        for kb in range(3):
            us = up[:, :, ka:ka + (hv - 1) * st + 1:st, kb:kb + (wv - 1) * st + 1:st]
            a[..., ka, kb] = torch.einsum("nchw,ndhw->ncd", us, v)
    return a


WGRAD_CASES = [
    # n, cu, cv, hv, wv, stride, pad, sum_n
    (2, 40, 136, 32, 32, 1, 1, 0),         # ragged cu / cv (vectorised partial stores), row slices -> workspace
    (2, 40, 136, 32, 32, 1, 1, 1),
    (3, 33, 130, 16, 48, 2, 0, 0),         # stride 2 on a (2H+1) grid; cv % 4 != 0 -> scalar partial stores and reduce
    (3, 33, 130, 16, 48, 2, 0, 1),
    (2, 7, 5, 17, 23, 1, 1, 1),            # tiny ragged tile, odd widths
    (2, 300, 1700, 6, 6, 1, 1, 0),         # >= 256 tiles: one slice, no workspace
    (1, 36, 40, 1, 40, 1, 1, 0),           # one V row: one part, no workspace
    (4, 36, 40, 1, 40, 2, 0, 1),           # one V row summed over samples: a workspace again
]


def test_wgrad_cases_cover_both_workspace_forms():
    """The cases above reach both forms of nb_conv2d_wgrad_h3_ws (one part written straight into the output, and partial
    blocks in a workspace + the fixed-order reduce), so the workspace refusal and the reduce keep being exercised."""
    need = [int(_lib.lib().nb_conv2d_wgrad_h3_ws_bytes(c[0], c[1], c[2], c[3], c[7])) for c in WGRAD_CASES]
    assert any(b == 0 for b in need) and any(b > 0 for b in need), need


@pytest.mark.parametrize("case", WGRAD_CASES, ids=lambda c: "n{}_cu{}_cv{}_{}x{}_s{}p{}_sum{}".format(*c))
def test_wgrad_h3_ws_vs_float64(dev, case):
    """nb_conv2d_wgrad_h3_ws with absmax slots (what ops._wgrad_launch runs): per-sample and summed results, with and without the
    slice workspace, against float64; the sample operands span 2^-20 .. 1 so the subnormal floor is exercised; a too-small
    workspace is refused; two runs are bit-identical (fixed-order reduce)."""
    n, cu, cv, hv, wv, st, pad, sum_n = case
    lib = _lib.lib()
    hu, wu = (hv, wv) if st == 1 else (2 * hv + 1, 2 * wv + 1)
    g = torch.Generator().manual_seed(sum(case))
    u = torch.randn([n, cu, hu, wu], generator=g)
    v = torch.randn([n, cv, hv, wv], generator=g)
    v[0] *= 2.0 ** -20                                         # a sample far below the range the scale is set by
    if n > 1:
        u[1] *= 2.0 ** -9
    ud, vd = u.to(dev), v.to(dev)
    u64, v64 = u.double(), v.double()
    want = wgrad_ref(u64, v64, st, pad)
    S = wgrad_ref(u64.abs(), v64.abs(), st, pad)
    su, sv = pow2_scale(1024.0, float(u.abs().max())) / 2, pow2_scale(1024.0, float(v.abs().max())) / 2   # (/2: log2f rounding)
    floor = SUB * (v64.abs().sum(dim=[2, 3])[:, None, :, None, None] / su + u64.abs().sum(dim=[2, 3])[:, :, None, None, None] / sv)
    L = (n if sum_n else 1) * hv * wv
    if sum_n:
        want, S, floor = want.sum(0), S.sum(0), floor.sum(0)
    tol = (L + 16) * U * S + floor
    u_bad = u64.clone()
    u_bad[:, 0] = 0
    bad = wgrad_ref(u_bad, v64, st, pad)
    catches(want, bad.sum(0) if sum_n else bad, tol, f"wgrad {case}")

    need = int(lib.nb_conv2d_wgrad_h3_ws_bytes(n, cu, cv, hv, sum_n))
    out_shape = ([] if sum_n else [n]) + [cu, cv, 3, 3]
    a = Out(out_shape, dev)
    ws = Out([max(need // 4, 1)], dev)
    slots = absmax_slots(dev, ud, None, vd)
    if need:
        rc = lib.nb_conv2d_wgrad_h3_ws(P(ud), P(vd), P(slots), 1, P(a.t), P(ws.t), need - 4, sum_n, n, cu, hu, wu, cv, hv, wv, st, pad,
                                       stream())
        assert rc != 0, "a workspace 4 bytes short was accepted"
        rc = lib.nb_conv2d_wgrad_h3_ws(P(ud), P(vd), P(slots), 1, P(a.t), None, 0, sum_n, n, cu, hu, wu, cv, hv, wv, st, pad, stream())
        assert rc != 0, "a missing workspace was accepted"
        torch.cuda.synchronize()
        assert torch.isnan(a.t).all(), "a refused call wrote its output"
    runs = []
    for _ in range(2):
        a.reset()
        ws.reset()
        _lib.check(lib.nb_conv2d_wgrad_h3_ws(P(ud), P(vd), P(slots), 1, P(a.t), P(ws.t) if need else None, need, sum_n,
                                             n, cu, hu, wu, cv, hv, wv, st, pad, stream()), "wgrad_h3_ws")
        torch.cuda.synchronize()
        assert a.guards_untouched() and ws.guards_untouched(), f"wgrad {case}: stray write"
        runs.append(a.t.clone())
    within(runs[0], want, tol, f"wgrad {case}")
    assert torch.equal(runs[0], runs[1]), f"wgrad {case}: two runs differ (the reduce is documented as fixed-order)"


def test_wgrad_h3_ws_explicit_scales(dev):
    """scales_are_absmax = 0: the two powers of two given directly (2^3 for u, 2^-5 for v) instead of max-abs slots."""
    n, cu, cv, h, w = 2, 24, 72, 16, 32
    g = torch.Generator().manual_seed(11)
    u, v = torch.randn([n, cu, h, w], generator=g) * 8, torch.randn([n, cv, h, w], generator=g) * 3e3
    lib = _lib.lib()
    want = wgrad_ref(u.double(), v.double(), 1, 1)
    S = wgrad_ref(u.double().abs(), v.double().abs(), 1, 1)
    sc = torch.tensor([2.0 ** 3, 2.0 ** -5], device=dev)
    ud, vd = u.to(dev), v.to(dev)                                     # (kept alive until the kernel has run)
    floor = SUB * (v.double().abs().sum(dim=[2, 3])[:, None, :, None, None] / 8 + u.double().abs().sum(dim=[2, 3])[:, :, None, None, None] * 32)
    tol = (h * w + 16) * U * S + floor
    need = int(lib.nb_conv2d_wgrad_h3_ws_bytes(n, cu, cv, h, 0))
    a, ws = Out([n, cu, cv, 3, 3], dev), Out([max(need // 4, 1)], dev)
    _lib.check(lib.nb_conv2d_wgrad_h3_ws(P(ud), P(vd), P(sc), 0, P(a.t), P(ws.t), need, 0, n, cu, h, w, cv, h, w, 1, 1,
                                         stream()), "wgrad_h3_ws")
    torch.cuda.synchronize()
    within(a.t, want, tol, "wgrad explicit scales")
    assert a.guards_untouched() and ws.guards_untouched()


# ---------------------------------------------------------------------------------------------------------------------
# nb_modconv_bwd_dot_f32 / nb_modconv_bwd_finish_f32
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("noise_kind", ["none", "shared", "per_sample"])
@pytest.mark.parametrize("hw", [(32, 32), (31, 33), (128, 128)])
def test_modconv_bwd_dot_vs_float64(dev, noise_kind, hw):
    """dd[n,o] = sum_p dy (y - noise): noise NULL, one plane for all samples (stride 0) and one per sample; hw % 4 == 0 (vector
    loads) and != 0.  Bound: hw products, each of a rounded difference -> (hw + 4) U sum|dy| |y - noise|."""
    n, o = (3, 40) if hw[0] < 128 else (4, 130)
    npx = hw[0] * hw[1]
    g = torch.Generator().manual_seed(npx + len(noise_kind))
    dy = (torch.randn([n, o, npx], generator=g) + 1) * 1e-3           # (non-zero means: dd is not a random-signed sum, so a
    y = torch.randn([n, o, npx], generator=g) + 1                     #  lost plane stays visible against (hw + 4) U S at 128^2)
    nz = None if noise_kind == "none" else torch.randn([1 if noise_kind == "shared" else n, 1, npx], generator=g) * 5
    y64 = y.double() - (0 if nz is None else nz.double())
    want = (dy.double() * y64).sum(-1)
    tol = (npx + 4) * U * (dy.double().abs() * y64.abs()).sum(-1)
    dy_bad = dy.double().clone()
    dy_bad[:, 0] = 0
    catches(want, (dy_bad * y64).sum(-1), tol, "bwd_dot")
    out = Out([n, o], dev)
    stride = npx if noise_kind == "per_sample" else 0
    nzd = None if nz is None else nz.to(dev)
    dyd, yd = dy.to(dev), y.to(dev)
    _lib.check(_lib.lib().nb_modconv_bwd_dot_f32(P(dyd), P(yd), P(nzd), stride, P(out.t), n, o, npx, stream()), "bwd_dot")
    torch.cuda.synchronize()
    within(out.t, want, tol, f"bwd_dot {noise_kind} {hw}")
    assert out.guards_untouched()


def finish_ref(A, s, W, dq):
    """dW, ds of nb_modconv_bwd_finish_f32 (A as [n, o, c, 9]) and the float64 sums of |terms| of each."""
    W9 = W.reshape(W.shape[0], W.shape[1], 9)
    dw = torch.einsum("nc,noct->oct", s, A)
    Sw = torch.einsum("nc,noct->oct", s.abs(), A.abs())
    ds = torch.einsum("oct,noct->nc", W9, A)
    Ss = torch.einsum("oct,noct->nc", W9.abs(), A.abs())
    Sq = torch.zeros_like(Ss)
    if dq is not None:
        wsq = W9.square().sum(-1)                                            # [o, c]
        q = dq.t() @ s.square()                                              # [o, c]
        dw = dw + 2 * W9 * q[..., None]
        Sw = Sw + 2 * W9.abs() * (dq.abs().t() @ s.square())[..., None]
        ds = ds + 2 * s * (dq @ wsq)
        Sq = 2 * s.abs() * (dq.abs() @ wsq)
    return dw.reshape(W.shape), Sw.reshape(W.shape), ds, Ss, Sq


@pytest.mark.parametrize("layout", ["up1_nco", "up2_noc"])
@pytest.mark.parametrize("n,o,c,demod", [(3, 40, 36, True), (3, 40, 36, False), (8, 520, 515, True), (1, 7, 300, True)])
def test_modconv_bwd_finish_vs_float64(dev, layout, n, o, c, demod):
    """dW = sum_n s A + 2 W sum_n dq s^2 and ds = sum_{o,t} W A + 2 s sum_o dq Wsq in both stride layouts ops passes (up = 1:
    A [n][c][o][9]; up = 2: A [n][o][c][9]), dq NULL (no demodulation), ragged and large o / c.  Bounds: dW sums n terms of one
    product plus a second sum of n terms of three roundings, then two more: (n + 6) U S; ds sums 9 o products -- (9 o + 14) U
    S -- plus 2 s q, q a sum of o terms dq Wsq (Wsq 9 squares, 3 more roundings): (o + 16) U S_q."""
    g = torch.Generator().manual_seed(n * o + c)
    A = torch.randn([n, o, c, 9], generator=g)
    s = torch.randn([n, c], generator=g)
    W = torch.randn([o, c, 3, 3], generator=g)
    dq = torch.randn([n, o], generator=g) if demod else None
    A64, s64, W64 = A.double(), s.double(), W.double()
    dq64 = None if dq is None else dq.double()
    dw_w, Sw, ds_w, Ss, Sq = finish_ref(A64, s64, W64, dq64)
    tol_w, tol_s = (n + 6) * U * Sw, (9 * o + 14) * U * Ss + (o + 16) * U * Sq
    A_bad = A64.clone()
    A_bad[:, :, 0] = 0
    bw, _, bs, _, _ = finish_ref(A_bad, s64, W64, dq64)
    catches(dw_w, bw, tol_w, "finish dW")
    catches(ds_w, bs, tol_s, "finish ds")
    if layout == "up1_nco":
        Ad = A.permute(0, 2, 1, 3).contiguous().to(dev)                      # [n, c, o, 9]
        strides = (c * o * 9, 9, o * 9)
    else:
        Ad = A.contiguous().to(dev)
        strides = (o * c * 9, c * 9, 9)
    dw, ds = Out([o, c, 3, 3], dev), Out([n, c], dev)
    sd, Wd = s.to(dev), W.to(dev)
    dqd = None if dq is None else dq.to(dev)
    _lib.check(_lib.lib().nb_modconv_bwd_finish_f32(P(Ad), *strides, P(sd), P(Wd), P(dqd), P(dw.t), P(ds.t), n, o, c, stream()), "finish")
    torch.cuda.synchronize()
    what = f"finish {layout} n{n} o{o} c{c} demod{demod}"
    within(dw.t, dw_w, tol_w, what + " dW")
    within(ds.t, ds_w, tol_s, what + " ds")
    assert dw.guards_untouched() and ds.guards_untouched()
    # one output alone (the other pointer NULL)
    dw.reset()
    _lib.check(_lib.lib().nb_modconv_bwd_finish_f32(P(Ad), *strides, P(sd), P(Wd), P(dqd), P(dw.t), None, n, o, c, stream()), "finish")
    torch.cuda.synchronize()
    within(dw.t, dw_w, tol_w, what + " dW only")
    assert dw.guards_untouched()


# ---------------------------------------------------------------------------------------------------------------------
# nb_absmax_f32 + nb_pack_h2_ranged_f32, and nb_conv3x3_s2_valid_h3 on its operands
# ---------------------------------------------------------------------------------------------------------------------

def ranged_pack(dev, x, scale, slots, dco_in):
    """nb_pack_h2_ranged_f32 (target 16384, as ops) into NaN-guarded outputs; returns (h2 Out, dco Out)."""
    n, c, h, w = x.shape
    xh = Out(ops.h2_shape(n, c, h, w), dev, dtype=torch.float16)
    dco = Out(list(dco_in.shape), dev)
    _lib.check(_lib.lib().nb_pack_h2_ranged_f32(P(x), c, None, 0, P(scale), P(xh.t), n, h * w, P(slots), 16384.0, P(dco_in), P(dco.t),
                                                dco_in.numel(), stream()), "pack_h2_ranged")
    torch.cuda.synchronize()
    assert xh.guards_untouched() and dco.guards_untouched()
    return xh, dco


def h2_emulated(v, c8):
    """The H2 halves of fp32 values v [n, c, h, w] (zero channels up to 8 c8) as torch does them on the CPU: hi = f16(v),
    lo = f16(v - hi) -- the same two roundings as the kernel, so the comparison is bit for bit."""
    n, c, h, w = v.shape
    vp = torch.zeros([n, c8 * 8, h, w], dtype=torch.float32)
    vp[:, :c] = v
    vp = vp.reshape(n, c8, 8, h, w).permute(0, 1, 3, 4, 2)
    hi = vp.half()
    lo = (vp - hi.float()).half()
    return hi, lo


@pytest.mark.parametrize("kind", ["random", "all_zero", "zero_scale_slot", "second_slot_zero"])
def test_pack_h2_ranged_edges(dev, kind):
    """nb_absmax_f32 + nb_pack_h2_ranged_f32: the halves are f16(v), f16(v - hi) of v = x * scale * k bit for bit (k the power of
    two from the slots), k brings max|x| max|scale| into (2^12, 2^14], dco_out = dco_in / k exactly.  Edges: an all-zero tensor
    (finite coefficients, exact zeros), all-zero scales (slot 1 = 0 counts as "no second operand") and no second operand."""
    n, c, h, w = 3, 21, 9, 40                                                 # c % 8 != 0: padded channels must be zero
    g = torch.Generator().manual_seed(len(kind))
    x = torch.randn([n, c, h, w], generator=g) * 3e-5
    sc = torch.rand([n, c], generator=g) + 0.5
    if kind == "all_zero":
        x.zero_()
    if kind == "zero_scale_slot":
        sc.zero_()
    xd, scd = x.to(dev), sc.to(dev)
    slots = absmax_slots(dev, xd, None, None if kind == "second_slot_zero" else scd)
    dco_in = torch.rand([n, 50], generator=g) + 0.25
    xh, dco = ranged_pack(dev, xd, scd, slots, dco_in.to(dev))
    got = dco.t.cpu()
    assert torch.isfinite(got).all() and (got > 0).all(), f"{kind}: output coefficients not finite / positive"
    k = dco_in / got
    kk = float(k[0, 0])
    assert torch.equal(k, torch.full_like(k, kk)) and math.log2(kk) == round(math.log2(kk)), f"{kind}: dco_in / dco_out is not one power of two"
    m = float(x.abs().max()) * (float(sc.abs().max()) if kind not in ("second_slot_zero", "zero_scale_slot") else 1.0)
    if m > 0:
        assert 2.0 ** 12 < m * kk <= 2.0 ** 14, f"{kind}: range scale {kk} puts the maximum at {m * kk}"
    else:
        assert kk == 2.0 ** 100
    hi, lo = h2_emulated(x * (sc * np.float32(kk))[:, :, None, None], (c + 7) // 8)
    got = xh.t.cpu()
    assert torch.equal(got[:, :, 0], hi) and torch.equal(got[:, :, 1], lo), f"{kind}: H2 halves differ from f16(v), f16(v - hi)"
    if kind in ("all_zero", "zero_scale_slot"):
        assert (got.float() == 0).all()


def s2_valid_ref(x, w, isc):
    return F.conv2d(x * isc[:, :, None, None], w, stride=2)


@pytest.mark.parametrize("form", ["wide", "narrow"])
def test_conv3x3_s2_valid_h3_vs_float64(dev, form):
    """nb_conv3x3_s2_valid_h3 on a range-packed operand (ops._conv2d_s2_valid_h3): y = (sum x w + bias) * oscale with
    oscale = the per-sample output coefficients / k; both tile forms (wo % 32 == 0 && ho % 8 == 0; wo == 16 && ho % 16 == 0),
    ragged c_in / c_out, oscale rows longer than c_out.  Bound per output, scaled by |oscale_in|: 9 c_in split products (14 U:
    12 U + the rounding of x * scale * k) -> (9 c_in + 16) U S, plus the subnormal floors 2^-24 (sum|w| / k + sum|x|) (weights
    are packed unscaled), plus two roundings of the epilogue."""
    n, ci, co = 2, 40, 136
    ho, wo = (8, 32) if form == "wide" else (16, 16)
    h, w = 2 * ho + 1, 2 * wo + 1
    g = torch.Generator().manual_seed(ho + wo)
    x = torch.randn([n, ci, h, w], generator=g) * 1e-4
    x[1] *= 2.0 ** -8
    wt = torch.randn([co, ci, 3, 3], generator=g) * 0.2
    isc = torch.rand([n, ci], generator=g) + 0.5
    ostride = co + 5
    osc_in = torch.rand([n, ostride], generator=g) + 0.5
    bias = torch.randn([co], generator=g)
    xd = x.to(dev)
    iscd = isc.to(dev)
    slots = absmax_slots(dev, xd, None, iscd)
    xh, dco = ranged_pack(dev, xd, iscd, slots, osc_in.to(dev))
    k = float(osc_in[0, 0] / dco.t[0, 0].cpu())
    wh = ops.pack_conv_weight_h3_dev(wt.to(dev), co_align=128)
    bd = bias.to(dev)
    y = Out([n, co, ho, wo], dev)
    L = _lib.lib()
    rc = L.nb_conv3x3_s2_valid_h3(P(xh.t), ci, P(wh), P(bd), P(dco.t), co - 1, P(y.t), n, h, w, co, stream())
    assert rc != 0, "an oscale stride below c_out was accepted"
    _lib.check(L.nb_conv3x3_s2_valid_h3(P(xh.t), ci, P(wh), P(bd), P(dco.t), ostride, P(y.t), n, h, w, co, stream()), "s2_valid")
    torch.cuda.synchronize()
    x64, w64, i64 = x.double(), wt.double(), isc.double()
    o64 = osc_in.double()[:, :co, None, None]
    conv = s2_valid_ref(x64, w64, i64)
    want = (conv + bias.double()[None, :, None, None] / k) * o64
    S = s2_valid_ref(x64.abs(), w64.abs(), i64.abs())
    xs = F.conv2d((x64.abs() * i64[:, :, None, None]).sum(1, keepdim=True), torch.ones([1, 1, 3, 3], dtype=torch.float64), stride=2)
    floor = SUB * (w64.abs().sum(dim=[1, 2, 3])[None, :, None, None] / k + xs)
    tol = ((9 * ci + 16) * U * S + floor) * o64 + 2 * U * want.abs()
    x_bad = x64.clone()
    x_bad[:, 0] = 0
    catches(want, (s2_valid_ref(x_bad, w64, i64) + bias.double()[None, :, None, None] / k) * o64, tol, "s2_valid")
    within(y.t, want, tol, f"s2_valid {form}")
    assert y.guards_untouched()
