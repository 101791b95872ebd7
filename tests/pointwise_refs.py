"""float64 restatements of the two streaming operators of csrc/nb_ops.hip -- bias_act (forward and the two gradient modes) and
upfirdn2d (as a gather) -- with the fp32 error bound of every output, and the input builders that keep elements away from
the decisions the kernels take in fp32 arithmetic of their own.  TEST INFRASTRUCTURE: imported by
tests/test_hip_pointwise_f64.py (GPU) and pinned against the reference-generated vectors by tests/test_pointwise_refs_cpu.py.

Everything is plain torch in float64, so torch.autograd differentiates the restatements (grad = 0 of bias_act, upfirdn2d).
U = 2^-24 is the fp32 unit roundoff; ulp(v) is the spacing of fp32 numbers at |v| (between U|v| and 2U|v|)."""
import math

import numpy as np
import torch

U = 2.0 ** -24
ACTS = ["linear", "relu", "lrelu", "tanh", "sigmoid", "elu", "selu", "softplus", "swish"]
ACT_CODE = {a: i + 1 for i, a in enumerate(ACTS)}                  # NB_ACT_* of include/neube_hip.h
ACT_DEFAULTS = {"linear": (0.0, 1.0), "relu": (0.0, math.sqrt(2)), "lrelu": (0.2, math.sqrt(2)), "tanh": (0.0, 1.0),
                "sigmoid": (0.0, 1.0), "elu": (0.0, 1.0), "selu": (0.0, 1.0), "softplus": (0.0, 1.0), "swish": (0.0, math.sqrt(2))}
SELU_SCALE = 1.0507009873554804934193349852946
SELU_ALPHA = 1.6732632423543772848170429916717
# the shapes and settings tests/test_hip_pointwise_f64.py runs bias_act at (the CPU file checks the builders on the same)
SMALL_SIZES = (1, 3, 4, 5, 255, 256, 257, 1023, 1025)
BIAS_SHAPE = (5, 12, 6)                                            # bias steps 72, 6 and 1
ALIGN_SHAPE = (2, 8, 4, 4)
WRAP_SHAPES = ((3, 7, 317, 317), (2, 16, 512, 516))                # past 8192 * 256 scalar elements / 8192 * 256 * 4 vector elements
WRAP_ACTS = ("lrelu", "swish")
GAIN, CLAMP = 1.3, 1.1
# K: ulps granted to the device's expf / tanhf / expm1f / log1pf per activation and mode (grad 0, 1, 2) = 4 x the largest error
# of the fp32 host oracle beyond the conditioning terms, at least 4 (tests/test_pointwise_refs_cpu.py measures it and explains
# why the gradient modes of sigmoid / softplus / swish take the forward's figure).  linear, relu and lrelu call no math
# function in any mode: K = 0, their bound is the counted roundings alone.
K_ULPS = {a: (4, 4, 4) for a in ACTS}
K_ULPS["swish"] = (6, 6, 6)
for _a in ("linear", "relu", "lrelu"):
    K_ULPS[_a] = (0, 0, 0)


def seed_of(shape, dim, act):
    return (int(np.prod(shape)) * 31 + (7 if dim is None else dim) * 5 + ACT_CODE[act]) % (2 ** 31)


KINK = 1e-3                       # half width of the neighbourhoods the input builders keep clear
# swish, grad 2: the kernel (like the reference's bias_act.cu:127) divides by d*d*d, d = exp(xr) + 1, which overflows fp32 for
# xr > 29.58 (d > cbrt(FLT_MAX) = 6.98e12) and turns the quotient into 0; past xr = 40 both return 0 outright.  The exact factor
# there is (2 - xr) / exp(xr) up to 1e-12 relative, at most 27.6 / 6.98e12 < 4e-12 in magnitude: an absolute term of the bound.
SWISH_G2_OVERFLOW_XR = 29.5
SWISH_G2_OVERFLOW_ABS = 4e-12
# rounded fp32 operations (beyond those inside the conditioning term) between the operands and the result, per activation:
#   forward: x + b is inside the conditioning term; linear / relu: * gain (1); lrelu: * alpha, * gain (2); the others: * gain (1)
#            [selu: + 3 for the product of the two fp32 constants]
#   grad 1 / grad 2: y = nb_act_grad(g, ..) * (gain * dy): gain * dy (1) and that product (1) for every activation, plus the
#            products / quotients of nb_act_grad's own line (the roundings of forming F are in F's error term dF, not here):
#     linear   g                                   0       -> 2, 2        relu   g or 0                       0 -> 2, 2
#     lrelu    g * alpha                           1       -> 3, 3
#     tanh     d = g * (1 - yy yy)                 1       -> 3;          d * (-2 yy)  (2 yy is exact)       +1 -> 4
#     sigmoid  d = (g * yy) * (1 - yy)             2       -> 4;          d * (1 - 2 yy)                     +1 -> 5
#     elu      g * (yy + 1)                        1       -> 3, 3        selu   g * scale or g * (yy + sa)   1 -> 3, 3
#     softplus g * (1 - c)                         1       -> 3;          (g * c) * (1 - c)                   2 -> 4
#     swish    ((g * c) * (xr + d)) / (d * d)      4       -> 6;          ((g * c) * n) / ((d * d) * d)       5 -> 7
FWD_ROUNDINGS = {"linear": 1, "relu": 1, "lrelu": 2, "tanh": 1, "sigmoid": 1, "elu": 1, "selu": 4, "softplus": 1, "swish": 1}
GRAD_ROUNDINGS = {"linear": (2, 2), "relu": (2, 2), "lrelu": (3, 3), "tanh": (3, 4), "sigmoid": (4, 5), "elu": (3, 3), "selu": (3, 3),
                  "softplus": (3, 4), "swish": (6, 7)}


def f32(v):
    """The float a C `float` parameter holds."""
    return float(np.float32(v))


def ulp(v):
    """Spacing of fp32 numbers at |v| (float64 tensor); 2^-149 below the smallest normal."""
    _, e = torch.frexp(v.abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(v), (e - 24).clamp_min(-149))


def _dbl(t):
    return None if t is None else (t if t.dtype == torch.float64 else t.double())


def _act(u, act, alpha):
    if act == "linear":
        return u
    if act == "relu":
        return torch.where(u > 0, u, torch.zeros_like(u))
    if act == "lrelu":
        return torch.where(u > 0, u, u * alpha)
    if act == "tanh":
        return torch.tanh(u)
    if act == "sigmoid":
        return 1 / (1 + torch.exp(-u))
    if act == "elu":
        return torch.where(u >= 0, u, torch.expm1(u.clamp(max=0)))
    if act == "selu":
        return torch.where(u >= 0, SELU_SCALE * u, SELU_SCALE * SELU_ALPHA * torch.expm1(u.clamp(max=0)))
    if act == "softplus":
        return torch.logaddexp(u, torch.zeros_like(u))              # (the kernel's x > 20 ? x : ... is within exp(-20) of it)
    if act == "swish":
        return u / (1 + torch.exp(-u))
    raise ValueError(act)


def _act_slope(u, act, alpha):
    """|d act / du| in float64 (the conditioning of the forward on the rounded x + b)."""
    one = torch.ones_like(u)
    if act == "linear":
        return one
    if act == "relu":
        return (u > 0).double()
    if act == "lrelu":
        return torch.where(u > 0, one, one * abs(alpha))
    if act == "tanh":
        return 1 - torch.tanh(u) ** 2
    s = torch.sigmoid(u)
    if act == "sigmoid":
        return s * (1 - s)
    if act == "elu":
        return torch.where(u >= 0, one, torch.exp(u.clamp(max=0)))
    if act == "selu":
        return torch.where(u >= 0, SELU_SCALE * one, SELU_SCALE * SELU_ALPHA * torch.exp(u.clamp(max=0)))
    if act == "softplus":
        return s
    return (s + u * s * (1 - s)).abs()                              # swish


def bias_index(numel, size_b, step_b):
    return (torch.arange(numel) // step_b) % size_b


def bias_act_ref(x, b, xref, yref, dy, grad, act, alpha, gain, clamp, step_b=1, K=None):
    """The three modes of nb_bias_act_grad_f32 (comment block at the head of the bias_act section of nb_ops.hip) in float64, on
    the operands the kernel gets; element i takes b[(i / step_b) % len(b)].  alpha, gain, clamp are rounded to float first.
      grad 0: y = clamp(act(x + b) * gain)
      grad 1: y = x * act'(.) * gain [* dy], 0 where the forward clamped
      grad 2: y = x * dy * act''(.) * gain, 0 where the forward clamped
    act' / act'' are functions of yy = yref / gain (0 when gain == 0, as the kernel substitutes) for every activation but swish,
    which takes xr = xref + b.  "Clamped" (yref, or swish's recomputed forward, not strictly inside +-clamp) and the branch of
    relu / lrelu / elu / selu (sign of yy) are read off the same fp32 yref / xref values the kernel reads.

    With K (ulps granted to the device's expf / tanhf / expm1f / log1pf; 0 for linear / relu / lrelu, whose bound is then
    k U (|x| + |b|) |gain| with k = 2, 2, 3 forward and k U |y| with k = 2, 2, 3 in grad 1) also returns the bound of every element.
    softplus and swish are granted the expf allowance twice in the gradient modes, on purpose: once as the relative error 2 K U
    of c = expf(.) carried through dF (a conditioning term: it is amplified where 1 - c or the swish numerators cancel), and once
    as K ulp(y) on the result, as for every activation that calls a math function.
      grad 0: |act'(x + b)| U (|x| + |b|) |gain|  (the rounding of x + b carried through)  + FWD_ROUNDINGS U |y| + K ulp(y)
      grad > 0: U |x gain dy| dF + GRAD_ROUNDINGS U |y| + K ulp(y), dF = the error of the factor F = act' or act'' in units of U,
                derived at each activation below from the roundings of yy (|yy|: the division by gain) and xr (|xref| + |b|)."""
    alpha, gain, clamp = f32(alpha), f32(gain), f32(clamp)
    x, b, xref, yref, dy = _dbl(x), _dbl(b), _dbl(xref), _dbl(yref), _dbl(dy)
    shape = x.shape
    bb = torch.zeros((), dtype=torch.float64) if b is None or b.numel() == 0 else b[bias_index(x.numel(), b.numel(), step_b)].reshape(shape)
    if grad == 0:
        u = x + bb
        y = _act(u, act, alpha) * gain
        if clamp >= 0:
            y = y.clamp(-clamp, clamp)
        if K is None:
            return y
        with torch.no_grad():
            tol = _act_slope(u, act, alpha) * U * (x.abs() + bb.abs()) * abs(gain) + FWD_ROUNDINGS[act] * U * y.abs() + K * ulp(y)
            if act == "softplus":
                tol = tol + torch.where(u > 20, torch.exp(-u.clamp(min=20)), torch.zeros_like(u)) * abs(gain)
        return y, tol
    assert grad in (1, 2)
    G1 = grad == 1
    g = x
    zero, one = torch.zeros_like(g), torch.ones_like(g)
    yy = (yref / gain if gain != 0 else zero) if yref is not None else zero
    ey = yy.abs()                                                   # error of yy in units of U (one division)
    Kc = 0 if K is None else 2 * K                                  # K ulps of expf as a relative error in units of U
    if act == "linear":
        F, dF = (one if G1 else zero), zero
    elif act == "relu":
        F, dF = (torch.where(yy > 0, one, zero) if G1 else zero), zero
    elif act == "lrelu":
        F, dF = (torch.where(yy > 0, one, one * alpha) if G1 else zero), zero
    elif act == "tanh":
        F = 1 - yy * yy                                             # yy*yy: 2 |yy| ey + yy^2; the subtraction: |F|
        dF = 3 * yy * yy + F.abs()
        if not G1:
            dF = dF * 2 * yy.abs() + F.abs() * 2 * ey               # F * (-2 yy)
            F = F * (-2 * yy)
    elif act == "sigmoid":
        om = 1 - yy                                                 # error ey + |om|
        F = yy * om
        dF = om.abs() * ey + yy.abs() * (ey + om.abs())
        if not G1:
            t = 1 - 2 * yy                                          # error 2 ey + |t|
            dF = dF * t.abs() + F.abs() * (2 * ey + t.abs())
            F = F * t
    elif act == "elu":
        neg = yy < 0
        F = torch.where(neg, yy + 1, one if G1 else zero)           # yy + 1: ey + |F|
        dF = torch.where(neg, ey + (yy + 1).abs(), zero)
    elif act == "selu":
        neg = yy < 0
        sa = SELU_SCALE * SELU_ALPHA                                # (fp32: two rounded constants and their rounded product: 3 sa)
        F = torch.where(neg, yy + sa, SELU_SCALE * one if G1 else zero)
        dF = torch.where(neg, ey + 3 * sa + (yy + sa).abs(), SELU_SCALE * one if G1 else zero)
    elif act == "softplus":
        c = torch.exp(-yy)                                          # relative error ey + Kc
        om = -torch.expm1(-yy)                                      # 1 - c without float64's own cancellation at small yy
        dc = c * (ey + Kc)
        F, dF = om, dc + om.abs()
        if not G1:
            F, dF = c * om, om.abs() * dc + c * dF
    elif act == "swish":
        xr = xref + bb
        exr = xref.abs() + bb.abs()                                 # error of xr in units of U
        big = xr > 40
        xs = xr.clamp(max=40)
        c = torch.exp(xs)                                           # relative error exr + Kc
        d = c + 1
        rd = exr + Kc + 1                                           # relative error of d (c < d), its own rounding included
        if G1:
            n = xs + d                                              # error exr + d rd + |n|
            F = torch.where(big, one, c * n / (d * d))
            dF = torch.where(big, zero, F.abs() * (exr + Kc + 2 * rd) + c / (d * d) * (exr + d * rd + n.abs()))
        else:
            n = xs * (2 - d) + 2 * d
            dn = exr * (2 - d).abs() + xs.abs() * (d * rd + (2 - d).abs()) + (xs * (2 - d)).abs() + 2 * d * rd + n.abs()
            F = torch.where(big, zero, c * n / (d * d * d))
            dF = torch.where(big, zero, F.abs() * (exr + Kc + 3 * rd) + c / (d * d * d) * dn)
    else:
        raise ValueError(act)
    scale = gain * (dy if dy is not None else one)
    y = g * F * scale
    keep = None
    if clamp >= 0:
        yf = _act(xref + bb, "swish", 0.0) * gain if act == "swish" else yref
        keep = (yf > -clamp) & (yf < clamp)
        y = torch.where(keep, y, zero)
    if K is None:
        return y
    tol = U * (g * scale).abs() * dF + GRAD_ROUNDINGS[act][grad - 1] * U * y.abs() + K * ulp(y)
    if act == "swish" and not G1:
        tol = tol + torch.where(xr > SWISH_G2_OVERFLOW_XR, SWISH_G2_OVERFLOW_ABS * (g * scale).abs(), zero)
    if keep is not None:
        tol = torch.where(keep, tol, zero)
    return y, tol


def _offenders(x, bb, act, alpha, gain, clamp):
    """Elements of x (float64 view of fp32 values) at a decision the kernels take in their own fp32 arithmetic."""
    u = x + bb
    bad = torch.zeros_like(u, dtype=torch.bool)
    if act in ("relu", "lrelu", "elu", "selu"):
        bad |= u.abs() < KINK
    if act == "swish":
        bad |= (u - 40).abs() < KINK
    if clamp is not None and clamp >= 0:
        y = _act(u, act, f32(alpha)) * f32(gain)
        bad |= (y.abs() - f32(clamp)).abs() < KINK * f32(clamp)
    return bad


def count_offenders(x, b, step_b, act, alpha, gain, clamp):
    x = torch.as_tensor(x).double().flatten()
    bb = 0.0 if b is None else torch.as_tensor(b).double()[bias_index(x.numel(), len(b), step_b)]
    return int(_offenders(x, bb, act, alpha, gain, clamp).sum())


# a few values per tensor that reach the far branches: softplus past 20, swish past 40 and in the range where d^3 overflows,
# the saturated ends of tanh / sigmoid / elu (|x + b| stays below 70: expf(-x) finite)
SPECIALS = np.array([25.0, -25.0, 45.0, -45.0, 60.0, -60.0, 35.0, 19.5, 20.5, 39.5, 40.5, 0.0, 1e-4, -1e-4, 8.0, -8.0], np.float32)


def bias_act_inputs(shape, dim, act, alpha, gain, clamp, seed):
    """x (scale 2, SPECIALS sprinkled in), b along `dim` (None: no bias), dy and ddx as float32 arrays, with every element of x
    that sits inside an excluded neighbourhood (x + b within KINK of 0 for relu / lrelu / elu / selu, or of 40 for swish; the
    forward output within KINK relative of +-clamp) moved by 2 KINK until none is left: nothing is excluded from a comparison."""
    rs = np.random.RandomState(seed)
    shape = tuple(shape)
    n = int(np.prod(shape))
    x = (rs.randn(n) * 2).astype(np.float32)
    if n >= 4 * len(SPECIALS):
        x[rs.choice(n, len(SPECIALS), replace=False)] = SPECIALS
    b = None if dim is None else rs.randn(shape[dim]).astype(np.float32)
    step_b = 1 if dim is None else int(np.prod(shape[dim + 1:]))
    xt = torch.from_numpy(x)
    bb = 0.0 if b is None else torch.from_numpy(b).double()[bias_index(n, len(b), step_b)]
    for _ in range(16):
        bad = _offenders(xt.double(), bb, act, alpha, gain, clamp)
        if not bad.any():
            break
        xt[bad] += np.float32(2 * KINK)
    dy = rs.randn(n).astype(np.float32)
    ddx = rs.randn(n).astype(np.float32)
    return xt.numpy().reshape(shape), b, dy.reshape(shape), ddx.reshape(shape), step_b


# ---------------------------------------------------------------------------------------------------------------------
# upfirdn2d
# ---------------------------------------------------------------------------------------------------------------------

def upfirdn2d_out_size(in_h, in_w, fh, fw, upx, upy, downx, downy, px0, px1, py0, py1):
    return (in_h * upy + py0 + py1 - fh + downy) // downy, (in_w * upx + px0 + px1 - fw + downx) // downx


def _taps(n_out, n_in, n_f, up, down, pad0):
    """For every filter tap t and output position o: the input index the tap meets (clamped) and whether it meets one: the
    position o * down - pad0 + t in the zero-stuffed image must be a multiple of `up` and inside the image."""
    o = torch.arange(n_out)[None, :]
    t = torch.arange(n_f)[:, None]
    u = o * down - pad0 + t
    i = torch.div(u, up, rounding_mode="floor")
    ok = (u >= 0) & (u % up == 0) & (i < n_in)
    return i.clamp(0, n_in - 1), ok


def upfirdn2d_ref(x, f, up=(1, 1), down=(1, 1), padding=(0, 0, 0, 0), flip=False, gain=1.0, bound=False):
    """y[m, oy, ox] = gain * sum_{fy, fx} x[m, iy, ix] * f'[fy, fx] over the taps whose position in the zero-stuffed image,
    (oy * downy - pady0 + fy, ox * downx - padx0 + fx), is a multiple of (upy, upx) and inside the image; f' is f flipped unless
    `flip` (upfirdn2d.cu's generic kernel, quoted at the head of the upfirdn2d section of nb_ops.hip).  x: [major, in_h, in_w] or
    NCHW, f: [fh, fw]; up / down = (x, y); padding = [x0, x1, y0, y1].  A gather in float64: differentiable in x.
    bound=True also returns (T + 2) U S per output: S = the same sum over absolute values, T = the number of taps that meet a
    sample for that output (T - 1 additions, the product and the rounding of f * gain).  T = 0 gives an exact 0."""
    upx, upy = up
    downx, downy = down
    px0, px1, py0, py1 = padding
    gain = f32(gain)
    x = _dbl(x)
    f = _dbl(f)
    lead = x.shape[:-2]
    in_h, in_w = x.shape[-2:]
    fh, fw = f.shape
    oh, ow = upfirdn2d_out_size(in_h, in_w, fh, fw, upx, upy, downx, downy, px0, px1, py0, py1)
    assert oh >= 1 and ow >= 1
    ff = f if flip else f.flip([0, 1])
    iy, oky = _taps(oh, in_h, fh, upy, downy, py0)
    ix, okx = _taps(ow, in_w, fw, upx, downx, px0)
    xm = x.reshape(-1, in_h, in_w)
    outs = [xm] + ([xm.detach().abs()] if bound else [])
    res = []
    for k, src in enumerate(outs):
        fk = ff.abs() if k else ff
        y = torch.zeros(src.shape[0], oh, ow, dtype=torch.float64)
        for fy in range(fh):
            if not oky[fy].any():
                continue
            rows = src.index_select(1, iy[fy]) * oky[fy].double()[None, :, None]
            for fx in range(fw):
                if not okx[fx].any() or float(fk[fy, fx]) == 0.0:
                    continue
                w = (okx[fx].double() * fk[fy, fx])[None, None, :]
                y = y + rows.index_select(2, ix[fx]) * w if src.requires_grad else y.addcmul_(rows.index_select(2, ix[fx]), w)
        res.append((y * (abs(gain) if k else gain)).reshape(*lead, oh, ow))
    if not bound:
        return res[0]
    T = oky.double().sum(0)[:, None] * okx.double().sum(0)[None, :]
    return res[0], (T + 2) * U * res[1]
