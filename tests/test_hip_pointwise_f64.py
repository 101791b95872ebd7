"""GPU: the two streaming operators of csrc/nb_ops.hip -- nb_bias_act_grad_f32 / nb_bias_act_f32 and nb_upfirdn2d_f32 -- through
their C entries on tensors built here, elementwise against the float64 restatements of tests/pointwise_refs.py (pinned on the
CPU by tests/test_pointwise_refs_cpu.py), past the grid caps of their launches; then the autograd wrappers ops.bias_act /
ops.upfirdn2d at the same shapes.  Every output of a C entry lies in a NaN-filled buffer with 64 guard floats on either side.

Bounds (U = 2^-24; ulp(v) = spacing of fp32 at |v|; all terms evaluated in float64 per element, pointwise_refs.bias_act_ref):
  bias_act grad 0: |act'(x + b)| U (|x| + |b|) |gain| carries the one rounding of x + b through the activation, then k U |y| for
    the k rounded products behind it -- linear, relu: k = 1 (* gain), i.e. 2 U (|x| + |b|) |gain| in all; lrelu: k = 2 (* alpha,
    * gain), 3 U (|x| + |b|) |gain| in all; tanh, sigmoid, elu, softplus, swish: k = 1; selu: k = 4 (the product of its two
    rounded constants) -- plus K ulp(y) for the device's tanhf / expf / expm1f / log1pf.  softplus adds exp(-x) |gain| past
    x = 20, where the kernel returns x.
  bias_act grad 1 / 2: y = g F gain dy with F = act' / act'' formed from yy = yref / gain (one rounding: |yy| U) or, for swish,
    xr = xref + b ((|xref| + |b|) U).  U |g gain dy| dF + k U |y| + K ulp(y), where dF (in U) follows the kernel's expression
    term by term -- tanh: 1 - yy yy has 3 yy^2 + |F| (this is the cancellation near saturation: an absolute 3 U on a factor that
    tends to 0), times 2 |yy| plus 2 |F| |yy| for grad 2; sigmoid: yy (1 - yy) has 2 |yy| |1 - yy| + yy^2; elu / selu below 0:
    |yy| + |F| (+ 3 scale alpha for selu's constants); softplus: c = expf(-yy) has c (|yy| + 2 K), 1 - c adds |1 - c|; swish:
    c = expf(xr) has c (|xr|.. + 2 K), d = c + 1, and the numerators xr + d and xr (2 - d) + 2 d carry their own cancellation --
    and k counts the remaining products and quotients (linear, relu 2; lrelu, elu, selu 3; tanh 3 / 4; sigmoid 4 / 5; softplus
    3 / 4; swish 6 / 7; spelled out line by line at GRAD_ROUNDINGS in pointwise_refs.py).  swish grad 2 adds 4e-12 |g gain dy| where xr > 29.5: d d d overflows fp32 there and the kernel, like
    the reference's, returns 0 for a factor of (2 - xr) / exp(xr).  Where the forward clamped the result is exactly 0.
  K: 0 for linear, relu and lrelu in every mode -- they call no math function, so the '... in all' figures above (and k U |y|,
    k = 2, 2, 3, in grad 1; an exact 0 in grad 2) are their whole bound.  For the others 4 x the largest error of the fp32 host
    oracle (oracle.neube_oracle.bias_act on float32, torch.autograd for the gradient modes) against the restatement beyond the
    terms above, at least 4.  Measured by tests/test_pointwise_refs_cpu.py (20000 elements, both clamp settings; the figures
    are those of one x86-64 host's libm, the CPU test re-measures and requires 4 m <= K <= max(4, ceil(8 m))), in ulps:
    forward  linear 0  relu 0  lrelu 0  tanh 0.32  sigmoid 0.69  elu 0.19  selu 0  softplus 0.50  swish 1.32  -> K = 4, swish 6;
    grad 1 / grad 2  linear, relu, lrelu: 0 / 0 -> K = 0;  tanh, elu, selu: 0 / 0 -> K = 4.
    sigmoid, softplus, swish grad 1 / 2: the host differentiates through its own ROUNDED forward (y (1 - y), 1 - 2 y with y
    one rounding off) and is 132 / 2415, 0 / 903 and 0 / 926 ulps from the restatement at |x| < 12, unboundedly more further
    out: the conditioning of the host's formula, not its math library.  The kernel's only math call in these modes is the
    expf whose host error the forward row measures, so they take the forward's K (4, 4, 6) instead of 4 x those figures.
    In the gradient modes of softplus and swish that allowance is granted twice on purpose: as the relative error 2 K U of
    c = expf(.) carried through dF, and as K ulp(y) on the result.
  upfirdn2d: (T + 2) U S per output, S = the float64 sum of |x f' gain| over the taps that meet a sample, T their number (T - 1
    additions, one product, the rounding of f' gain); an output whose window meets no sample is exactly 0.  dx through the
    wrapper is another launch with up and down swapped: (T' + 2) U S', T' = ceil(fh / downy) ceil(fw / downx), S' = the adjoint
    of the absolute values.  db: the per-element bounds summed plus L U sum|terms| for torch's fp32 sum of L elements.
A skipped grid-stride pass or plane leaves NaN; a wrong plane, flip or bias step moves outputs by ~their own size, 2^20 times
these bounds."""
import math

import numpy as np
import pytest
import torch

import pointwise_refs as pr
from brushstroke_engine_amd import _lib
from pointwise_refs import ACT_CODE, ACT_DEFAULTS, ACTS, CLAMP, GAIN, K_ULPS, U

pytestmark = pytest.mark.gpu
GUARD = 64                       # NaN floats before and after every output buffer (keeps 16-byte alignment)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


def P(t):
    return None if t is None else t.data_ptr()


def stream():
    return torch.cuda.current_stream().cuda_stream


class Out:
    """An output tensor of `shape` inside a NaN-filled buffer with GUARD elements on either side (`offset` floats further in:
    an output that is only 4-byte aligned)."""

    def __init__(self, shape, dev, offset=0):
        self.numel, self.off = int(np.prod(shape)), GUARD + offset
        self.buf = torch.full([self.numel + 2 * GUARD + offset], float("nan"), dtype=torch.float32, device=dev)
        self.t = self.buf[self.off:self.off + self.numel].view(shape)

    def guards_untouched(self):
        g = torch.cat([self.buf[:self.off], self.buf[self.off + self.numel:]])
        return bool(torch.isnan(g).all())

    def all_nan(self):
        return bool(torch.isnan(self.buf).all())

    def reset(self):
        self.buf.fill_(float("nan"))


def within(got, want, tol, what):
    """|got - want| <= tol elementwise (float64), and no NaN where a value is expected."""
    got = got.detach().double().cpu()
    want, tol = want.detach().double(), tol.detach().double()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert not torch.isnan(got).any(), f"{what}: {int(torch.isnan(got).sum())} outputs never written"
    d = (got - want).abs()
    bad = d > tol
    if bad.any():
        i = int(torch.nonzero(bad.flatten())[0])
        r = float((d / tol.expand_as(d).clamp_min(1e-300))[bad].max())
        raise AssertionError(f"{what}: {int(bad.sum())} of {d.numel()} outside the bound (worst {r:.3g}x); first at flat index {i}: "
                             f"got {float(got.flatten()[i]):.9g} want {float(want.flatten()[i]):.9g} "
                             f"tol {float(tol.expand_as(d).flatten()[i]):.3g}")


def misaligned(t, dev):
    """A copy of the device tensor t that starts one float past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 4, dtype=torch.float32, device=dev)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


# ---------------------------------------------------------------------------------------------------------------------
# bias_act through the C entry
# ---------------------------------------------------------------------------------------------------------------------

def ba_launch(out, x, b, xref, yref, dy, grad, act, alpha, gain, clamp, step_b):
    rc = _lib.lib().nb_bias_act_grad_f32(P(x), P(b), P(xref), P(yref), P(dy), P(out.t), x.numel(), 0 if b is None else b.numel(),
                                         step_b, grad, ACT_CODE[act], alpha, gain, clamp, stream())
    torch.cuda.synchronize()
    return rc


class BiasActCase:
    """One input set on the host and the device, with the float64 result and bound of the three modes.  yref is the float64
    forward rounded to fp32 on the host, so every operand of every launch is built here."""

    def __init__(self, shape, dim, act, clamp, dev, gain=GAIN):
        self.act, self.gain, self.clamp = act, gain, clamp
        self.alpha = ACT_DEFAULTS[act][0]
        x, b, dy, ddx, self.step_b = pr.bias_act_inputs(shape, dim, act, self.alpha, GAIN, CLAMP, seed=pr.seed_of(shape, dim, act))
        T = torch.from_numpy
        self.h = dict(x=T(x).flatten(), b=None if b is None else T(b), dy=T(dy).flatten(), ddx=T(ddx).flatten())
        cfg = dict(act=act, alpha=self.alpha, gain=gain, clamp=clamp, step_b=self.step_b)
        y64 = pr.bias_act_ref(self.h["x"], self.h["b"], None, None, None, 0, **cfg)
        self.h["yref"] = y64.float()
        self.d = {k: None if v is None else v.to(dev) for k, v in self.h.items()}
        self.cfg, self.dev, self.n = cfg, dev, self.h["x"].numel()

    def operands(self, grad, where):
        s = where
        return {0: (s["x"], s["b"], None, None, None), 1: (s["dy"], s["b"], s["x"], s["yref"], None),
                2: (s["ddx"], s["b"], s["x"], s["yref"], s["dy"])}[grad]

    def ref(self, grad):
        x, b, xref, yref, dy = self.operands(grad, self.h)
        return pr.bias_act_ref(x, b, xref, yref, dy, grad, K=K_ULPS[self.act][grad], **self.cfg)

    def run(self, grad, out=None, replace=None):
        x, b, xref, yref, dy = self.operands(grad, {**self.d, **(replace or {})})
        out = out or Out([self.n], self.dev)
        rc = ba_launch(out, x, b, xref, yref, dy, grad, self.act, self.alpha, self.gain, self.clamp, self.step_b)
        _lib.check(rc, "bias_act")
        return out

    def check(self, what):
        # bound per element (pointwise_refs.bias_act_ref): grad 0: |act'| U (|x| + |b|) |gain| + FWD_ROUNDINGS U |y| + K ulp(y), i.e.
        # k U (|x| + |b|) |gain| with k = 2 (linear, relu: x + b, * gain) or 3 (lrelu: + * alpha) and K = 0; grad 1 / 2:
        # U |g gain dy| dF + GRAD_ROUNDINGS U |y| + K ulp(y), k = 2 (linear, relu), 3 (lrelu, elu, selu), 3 / 4 (tanh, softplus),
        # 4 / 5 (sigmoid), 6 / 7 (swish), each count written out next to GRAD_ROUNDINGS
        for grad in (0, 1, 2):
            want, tol = self.ref(grad)
            out = self.run(grad)
            within(out.t, want, tol, f"{what} grad {grad}")
            assert out.guards_untouched(), f"{what} grad {grad}: stray write"


@pytest.mark.parametrize("act", ACTS)
def test_bias_act_small_shapes_vs_float64(dev, act):
    """All modes, clamp on and off: sizes around one workgroup and one vector without a bias (size_b = 0, b = NULL); (5, 12, 6)
    with the bias along each dimension (steps 72, 6, 1: the last two are no multiple of 4 and must take the scalar kernel
    although the size is one); (2, 8, 4, 4); gain = 0 in the gradient modes (yy = 0 on both sides)."""
    for clamp in (CLAMP, -1.0):
        for n in pr.SMALL_SIZES:
            BiasActCase((n,), None, act, clamp, dev).check(f"{act} clamp {clamp} n {n}")
        for dim in (0, 1, 2):
            BiasActCase(pr.BIAS_SHAPE, dim, act, clamp, dev).check(f"{act} clamp {clamp} bias dim {dim}")
        BiasActCase(pr.ALIGN_SHAPE, 1, act, clamp, dev).check(f"{act} clamp {clamp} {pr.ALIGN_SHAPE}")
        c = BiasActCase(pr.BIAS_SHAPE, 1, act, clamp, dev, gain=0.0)
        for grad in (1, 2):
            want, tol = c.ref(grad)
            assert float(want.abs().max()) == 0.0
            out = c.run(grad)
            within(out.t, want, tol, f"{act} gain 0 grad {grad}")
            assert out.guards_untouched()


@pytest.mark.parametrize("act", ACTS)
def test_bias_act_misaligned_pointer_equals_aligned_run(dev, act):
    """x, then y, then each of xref / yref / dy one float off a 16-byte boundary: the result (and the guards around a misaligned
    y) must equal the aligned run's bit for bit, which test_bias_act_small_shapes_vs_float64 holds against float64.  The launch
    is meant to take the scalar kernel here; the test cannot observe which kernel ran (a 16-byte access at a 4-byte aligned
    address returns the same values on this hardware), only that the answer and the written range are the same."""
    for clamp in (CLAMP, -1.0):
        c = BiasActCase(pr.ALIGN_SHAPE, 1, act, clamp, dev)
        base = {g: c.run(g).t.clone() for g in (0, 1, 2)}
        moved = {k: misaligned(c.d[k], dev) for k in ("x", "dy", "ddx", "yref")}
        # (the tensor in the kernel's x slot is x, dy, ddx for grad 0, 1, 2; xref is x for grad 1, 2; dy is dy for grad 2)
        runs = [(0, {"x": moved["x"]}, None), (1, {"dy": moved["dy"]}, None), (2, {"ddx": moved["ddx"]}, None),
                (0, {}, 1), (1, {}, 1), (2, {}, 1),
                (1, {"x": moved["x"]}, None), (2, {"x": moved["x"]}, None), (1, {"yref": moved["yref"]}, None),
                (2, {"yref": moved["yref"]}, None), (2, {"dy": moved["dy"]}, None)]
        for grad, rep, out_off in runs:
            out = Out([c.n], dev, offset=out_off or 0)
            c.run(grad, out=out, replace=rep)
            what = f"{act} clamp {clamp} grad {grad} moved {sorted(rep) or 'y'}"
            assert torch.equal(out.t, base[grad]), what
            assert out.guards_untouched(), what + ": stray write"


def test_bias_act_empty_and_refused_calls(dev):
    lib = _lib.lib()
    c = BiasActCase((256,), None, "swish", CLAMP, dev)
    b = torch.ones(4, device=dev)
    out = Out([256], dev)
    d = c.d
    for grad in (0, 1, 2):                                                # size_x = 0: NB_OK, nothing written
        rc = lib.nb_bias_act_grad_f32(P(d["x"]), None, P(d["x"]), P(d["yref"]), P(d["dy"]), P(out.t), 0, 0, 1, grad, ACT_CODE["swish"], 0.0, GAIN,
                                      CLAMP, stream())
        torch.cuda.synchronize()
        assert rc == _lib.NB_OK and out.all_nan(), grad
    sw, th = ACT_CODE["swish"], ACT_CODE["tanh"]
    refused = [  # (x, b, xref, yref, dy, size_b, step_b, grad, act code)
        (d["x"], None, d["x"], d["yref"], d["dy"], 0, 1, 3, sw),          # grad = 3
        (d["x"], None, None, None, None, 0, 1, -1, sw),
        (d["x"], None, None, None, None, 0, 1, 0, 0),                     # activation code out of range
        (d["x"], None, None, None, None, 0, 1, 0, 10),
        (d["dy"], None, None, d["yref"], None, 0, 1, 1, sw),              # swish grad 1 without xref
        (d["dy"], None, d["x"], None, None, 0, 1, 1, th),                 # tanh grad 1 without yref
        (d["x"], b, None, None, None, 4, 0, 0, sw),                       # a bias with step_b = 0
        (d["x"], None, None, None, None, 4, 64, 0, sw),                   # a bias size without a bias
    ]
    for x, bb, xref, yref, dy, size_b, step_b, grad, code in refused:
        rc = lib.nb_bias_act_grad_f32(P(x), P(bb), P(xref), P(yref), P(dy), P(out.t), 256, size_b, step_b, grad, code, 0.0, 1.0, CLAMP,
                                      stream())
        torch.cuda.synchronize()
        assert rc < 0 and out.all_nan(), (size_b, step_b, grad, code, rc)
    assert lib.nb_bias_act_grad_f32(None, None, None, None, None, P(out.t), 256, 0, 1, 0, sw, 0.0, 1.0, -1.0, stream()) < 0
    assert lib.nb_bias_act_f32(P(d["x"]), None, P(out.t), 256, 0, 1, 10, 0.0, 1.0, -1.0, stream()) < 0
    torch.cuda.synchronize()
    assert out.all_nan()
    # the forward-only entry is the same launch
    rc = lib.nb_bias_act_f32(P(d["x"]), None, P(out.t), 256, 0, 1, sw, 0.0, GAIN, CLAMP, stream())
    _lib.check(rc, "bias_act")
    torch.cuda.synchronize()
    assert torch.equal(out.t, c.run(0).t) and out.guards_untouched()


@pytest.mark.parametrize("clamp", [CLAMP, -1.0])
@pytest.mark.parametrize("act", pr.WRAP_ACTS)
@pytest.mark.parametrize("shape", pr.WRAP_SHAPES)
def test_bias_act_past_the_grid_cap_vs_float64(dev, shape, act, clamp):
    """The launch caps its grid at 8192 workgroups: (3, 7, 317, 317) = 2 110 269 elements (odd: the scalar kernel, 13 117 past
    8192 * 256) and (2, 16, 512, 516) = 8 454 144 (bias step 264 192: the vector kernel, 65 536 past 8192 * 256 * 4) make the
    grid-stride loop repeat.  Bias on dim 1, gain 1.3; lrelu reads yref, swish xref; all three modes."""
    n = int(np.prod(shape))
    assert n > 8192 * 256 * (4 if n % 4 == 0 else 1) and (n % 4 == 0) == (shape == pr.WRAP_SHAPES[1])
    c = BiasActCase(shape, 1, act, clamp, dev)
    assert c.step_b == shape[2] * shape[3] and all(t is None or t.data_ptr() % 16 == 0 for t in c.d.values())
    c.check(f"{act} clamp {clamp} {shape}")


# ---------------------------------------------------------------------------------------------------------------------
# upfirdn2d through the C entry
# ---------------------------------------------------------------------------------------------------------------------

# name: (major, in_h, in_w, fh, fw, (upx, upy), (downx, downy), [padx0, padx1, pady0, pady1]) -- every specialised launch of the
# switch in nb_upfirdn2d_f32, at one of two anchors worked through nb_upfirdn2d_launch_t:
#   output 48x40, major 1501: 8 workgroups per plane, 12 008 > 8192 -> gy = 751: planes 0-749 are walked twice, plane 750 once
#   output 128x128, major 259: 64 per plane, gy 259 -> 130 -> 65: planes 0-63 are walked four times, plane 64 three times
# with odd input extents (at down = 2, in * up - out * down is -1 or -3, never 0).
DISPATCH = {
    "1111_4x4":  (1501, 47, 41, 4, 4, (1, 1), (1, 1), [1, 1, 2, 2]),
    "1111_3x5":  (259, 129, 127, 3, 5, (1, 1), (1, 1), [2, 3, 1, 0]),
    "2211_4x4":  (1501, 23, 19, 4, 4, (2, 2), (1, 1), [3, 2, 2, 3]),
    "2211_1x1":  (259, 65, 63, 1, 1, (2, 2), (1, 1), [2, 0, -1, -1]),
    "2211_3x5":  (1501, 23, 21, 3, 5, (2, 2), (1, 1), [1, 1, 3, 1]),
    "1122_4x4":  (259, 253, 255, 4, 4, (1, 1), (2, 2), [2, 1, 3, 3]),
    "1122_3x5":  (1501, 95, 79, 3, 5, (1, 1), (2, 2), [2, 2, 1, 2]),
    "2111_1x12": (1501, 47, 21, 1, 12, (2, 1), (1, 1), [5, 4, 1, 0]),
    "1211_12x1": (259, 65, 127, 12, 1, (1, 2), (1, 1), [0, 1, 4, 5]),
    "1121_1x12": (1501, 49, 81, 1, 12, (1, 1), (2, 1), [5, 5, 0, -1]),
    "1112_12x1": (259, 257, 127, 12, 1, (1, 1), (1, 2), [1, 0, 5, 4]),
}
UP_GAIN = 1.7


def up_inputs(case, seed):
    major, ih, iw, fh, fw = case[:5]
    rs = np.random.RandomState(seed)
    x = torch.from_numpy(rs.randn(major, ih, iw).astype(np.float32))
    f = torch.from_numpy(rs.randn(fh, fw).astype(np.float32))              # asymmetric: a wrong flip moves every output
    return x, f


def up_launch(out, x, f, case, flip, gain=UP_GAIN):
    major, ih, iw, fh, fw, up, down, pad = case
    rc = _lib.lib().nb_upfirdn2d_f32(P(x), P(f), P(out.t), major, ih, iw, fh, fw, up[0], up[1], down[0], down[1], pad[0], pad[1], pad[2],
                                     pad[3], int(flip), gain, stream())
    torch.cuda.synchronize()
    return rc


def up_out_shape(case):
    major, ih, iw, fh, fw, up, down, pad = case
    return (major,) + pr.upfirdn2d_out_size(ih, iw, fh, fw, up[0], up[1], down[0], down[1], *pad)


def up_check(case, flip, dev, what, seed=0, generic_equal=False, gain=UP_GAIN):
    """One launch against float64; with generic_equal also the same launch under nb_debug_set_upfirdn_generic(1): the generic
    kernel walks the same taps in the same order, so against float64 again and bit for bit equal."""
    x, f = up_inputs(case, seed)
    want, tol = pr.upfirdn2d_ref(x, f, case[5], case[6], case[7], flip, gain, bound=True)
    xd, fd = x.to(dev), f.to(dev)
    out = Out(up_out_shape(case), dev)
    _lib.check(up_launch(out, xd, fd, case, flip, gain), "upfirdn2d")
    within(out.t, want, tol, what)
    assert out.guards_untouched(), what + ": stray write"
    if generic_equal:
        gen = Out(up_out_shape(case), dev)
        _lib.lib().nb_debug_set_upfirdn_generic(1)
        try:
            _lib.check(up_launch(gen, xd, fd, case, flip, gain), "upfirdn2d")
        finally:
            _lib.lib().nb_debug_set_upfirdn_generic(0)
        within(gen.t, want, tol, what + " (generic kernel)")
        assert gen.guards_untouched(), what + " (generic kernel): stray write"
        assert torch.equal(gen.t, out.t), what + ": generic and specialised kernels differ"
    return want, tol, out


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("name", list(DISPATCH))
def test_upfirdn2d_dispatch_table_vs_float64(dev, name, flip):
    case = DISPATCH[name]
    shape = up_out_shape(case)
    assert shape in ((1501, 48, 40), (259, 128, 128)), shape
    up_check(case, flip, dev, f"upfirdn2d {name} flip {flip}", seed=len(name) + sum(case[:5]))


def test_upfirdn2d_generic_kernel_vs_float64(dev):
    """The generic kernel: reached through factors >= 4 (up = 4 with a 4x4 filter, down = (1, 5), which would alias the dispatch
    key), and through the debug switch at 9 x 500 x 502 = 2 259 000 outputs (past 8192 * 256: its 64-bit stride loop repeats),
    where it must equal the specialised <2,2,1,1> 4x4 kernel bit for bit."""
    for flip in (False, True):
        up_check((3, 9, 13, 4, 4, (4, 4), (1, 1), [3, 3, 3, 3]), flip, dev, f"up 4 flip {flip}")
        up_check((3, 33, 17, 4, 4, (1, 1), (1, 5), [2, 2, 2, 2]), flip, dev, f"down (1, 5) flip {flip}")
        up_check((2, 17, 33, 3, 5, (2, 1), (5, 1), [2, 2, 2, 2]), flip, dev, f"up (2, 1) down (5, 1) flip {flip}")
    up_check((9, 250, 251, 4, 4, (2, 2), (1, 1), [2, 1, 2, 1]), False, dev, "9 x 250 x 251 up 2", generic_equal=True)


# (major <= 3) name: case
EDGES = {
    "in_w 1":              (3, 7, 1, 3, 5, (1, 1), (1, 1), [2, 2, 1, 1]),
    "in_w 1 up 2":         (2, 5, 1, 4, 4, (2, 2), (1, 1), [2, 1, 2, 1]),
    "in_h 1":              (3, 1, 9, 3, 5, (1, 1), (1, 1), [2, 2, 1, 1]),
    "in_h 1 down 2":       (3, 1, 9, 4, 4, (1, 1), (2, 2), [2, 2, 2, 2]),
    "1x1 output":          (2, 4, 4, 4, 4, (1, 1), (1, 1), [0, 0, 0, 0]),
    "1x1 output up 2":     (2, 2, 2, 4, 4, (2, 2), (1, 1), [0, 0, 0, 0]),
    "crop left / bottom":  (2, 9, 11, 3, 5, (1, 1), (1, 1), [-1, 2, 1, -2]),
    "crop right / top":    (2, 9, 11, 3, 5, (1, 1), (1, 1), [2, -1, -2, 1]),
    "crop all up 2":       (2, 9, 11, 4, 4, (2, 2), (1, 1), [-1, -2, -3, -1]),
    "crop all down 2":     (2, 19, 21, 4, 4, (1, 1), (2, 2), [-1, -2, -3, -1]),
    "wide border":         (1, 5, 6, 4, 4, (1, 1), (1, 1), [7, 6, 6, 7]),
    "wide border up 2":    (2, 5, 6, 4, 4, (2, 2), (1, 1), [9, 8, 8, 9]),
    "wide border down 2":  (2, 5, 6, 3, 5, (1, 1), (2, 2), [9, 8, 8, 9]),
    "pad 2 1 0 3":         (2, 9, 13, 3, 5, (1, 1), (1, 1), [2, 1, 0, 3]),
    "pad 2 1 0 3 up 2":    (2, 9, 13, 4, 4, (2, 2), (1, 1), [2, 1, 0, 3]),
    "filter 1x1":          (3, 6, 7, 1, 1, (1, 1), (1, 1), [1, 1, 0, 0]),
    "filter 3x5 up 2":     (3, 6, 7, 3, 5, (2, 2), (1, 1), [2, 2, 1, 1]),
    "filter 32x32":        (1, 9, 7, 32, 32, (1, 1), (1, 1), [16, 16, 16, 16]),
    "filter 32x32 up 2":   (1, 5, 5, 32, 32, (2, 2), (1, 1), [16, 16, 16, 16]),
    "filter 32x32 up 3":   (1, 5, 5, 32, 32, (3, 3), (1, 1), [16, 16, 16, 16]),
    "255 outputs":         (3, 15, 17, 3, 5, (1, 1), (1, 1), [2, 2, 1, 1]),
    "256 outputs":         (3, 16, 16, 3, 5, (1, 1), (1, 1), [2, 2, 1, 1]),
    "257 outputs":         (3, 1, 257, 3, 5, (1, 1), (1, 1), [2, 2, 1, 1]),
    "257 outputs 4x4":     (3, 1, 257, 4, 4, (1, 1), (1, 1), [2, 1, 2, 1]),
}


@pytest.mark.parametrize("name", list(EDGES))
def test_upfirdn2d_edges_vs_float64(dev, name):
    """Both flips, against float64 and against the generic kernel bit for bit; outputs whose window meets no sample (wide
    borders) have a bound of 0."""
    case = EDGES[name]
    for flip in (False, True):
        want, tol, _ = up_check(case, flip, dev, f"upfirdn2d {name} flip {flip}", seed=len(name), generic_equal=True, gain=0.7)
        if name.startswith("wide border"):
            assert int((tol == 0).sum()) > 0 and float(want[tol == 0].abs().max()) == 0.0
    px = {"255 outputs": 255, "256 outputs": 256, "257 outputs": 257}.get(name)
    assert px is None or int(np.prod(up_out_shape(case)[1:])) == px


def test_upfirdn2d_refused_calls(dev):
    ok = (2, 9, 11, 3, 5, (1, 1), (1, 1), [2, 2, 1, 1])
    x, f = (t.to(dev) for t in up_inputs((2, 40, 40, 33, 32), 1))
    out = Out([2, 64, 64], dev)

    def call(case, xx=x, ff=f, yy=out.t):
        major, ih, iw, fh, fw, up, down, pad = case
        rc = _lib.lib().nb_upfirdn2d_f32(P(xx), P(ff), P(yy), major, ih, iw, fh, fw, up[0], up[1], down[0], down[1], *pad, 0, 1.0, stream())
        torch.cuda.synchronize()
        return rc

    def variant(**kw):
        keys = ("major", "ih", "iw", "fh", "fw", "up", "down", "pad")
        d = dict(zip(keys, ok))
        d.update(kw)
        return tuple(d[k] for k in keys)

    assert call(ok, xx=None) < 0 and call(ok, ff=None) < 0 and call(ok, yy=None) < 0
    for case in (variant(fh=33, fw=32), variant(fh=0), variant(major=0), variant(ih=0), variant(up=(0, 1)), variant(up=(1, 0)),
                 variant(down=(0, 1)), variant(down=(1, 0)), variant(pad=[-5, -5, 1, 1]), variant(pad=[2, 2, -4, -4])):
        assert call(case) < 0 and out.all_nan(), case
    assert call(variant(fh=32, fw=32, pad=[16, 16, 16, 16])) == _lib.NB_OK


# ---------------------------------------------------------------------------------------------------------------------
# the autograd wrappers at the same shapes
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("act", pr.WRAP_ACTS)
def test_ops_bias_act_at_the_vector_wrap_shape_vs_float64_autograd(dev, act, order):
    """ops.bias_act at (2, 16, 512, 516), bias on dim 1, gain 1.3, clamp 1.1: y, dx, db (order 1) and d_dy, d_x, d_b (order 2)
    against torch.autograd in double on the grad-0 restatement.  lrelu's gradient reads only the sign of the saved y and
    swish's the saved x, so (inputs away from the kinks) the bounds are those of the kernel's modes on exact operands."""
    from brushstroke_engine_amd import ops
    shape = pr.WRAP_SHAPES[1]
    c = BiasActCase(shape, 1, act, CLAMP, dev)
    L = c.n // shape[1]
    red = [0, 2, 3]
    x, b, dy = (c.d[k].view(s).clone().requires_grad_(True) for k, s in (("x", shape), ("b", (shape[1],)), ("dy", shape)))
    y = ops.bias_act(x, b, dim=1, act=act, gain=GAIN, clamp=CLAMP)
    dx, db = torch.autograd.grad(y, [x, b], dy, create_graph=True)
    xr, br, dyr = (c.h[k].double().view(s).requires_grad_(True) for k, s in (("x", shape), ("b", (shape[1],)), ("dy", shape)))
    yr = pr.bias_act_ref(xr, br, None, None, None, 0, **c.cfg)
    dxr, dbr = torch.autograd.grad(yr, [xr, br], dyr, create_graph=True)
    if order == 1:
        for grad, got, want in ((0, y, yr), (1, dx, dxr)):
            again, tol = c.ref(grad)
            assert float((again.view(shape) - want.detach()).abs().max()) <= 1e-12 * float(want.detach().abs().max())
            within(got, want, tol.view(shape), f"ops.bias_act {act} {'y' if grad == 0 else 'dx'}")
            if grad == 1:
                within(db, dbr, tol.view(shape).sum(red) + L * U * want.detach().abs().sum(red), f"ops.bias_act {act} db")
        return
    ddx = c.d["ddx"].view(shape)
    d_dy, d_x, d_b = torch.autograd.grad((dx * ddx).sum(), [dy, x, b], allow_unused=True)
    g2 = torch.autograd.grad((dxr * c.h["ddx"].double().view(shape)).sum(), [dyr, xr, br], allow_unused=True)
    zero = lambda t, like: torch.zeros_like(like) if t is None else t
    cfg1 = dict(K=K_ULPS[act][1], **c.cfg)
    _, tol_ddy = pr.bias_act_ref(c.h["ddx"], c.h["b"], c.h["x"], c.h["yref"], None, 1, **cfg1)
    _, tol_dx = c.ref(2)
    within(zero(d_dy, dy), zero(g2[0], dyr), tol_ddy.view(shape), f"ops.bias_act {act} d_dy")
    within(zero(d_x, x), zero(g2[1], xr), tol_dx.view(shape), f"ops.bias_act {act} d_x")
    within(zero(d_b, b), zero(g2[2], br), tol_dx.view(shape).sum(red) + L * U * zero(g2[1], xr).detach().abs().sum(red),
           f"ops.bias_act {act} d_b")


@pytest.mark.parametrize("name", list(DISPATCH))
def test_ops_upfirdn2d_gradients_vs_float64_autograd(dev, name):
    """ops.upfirdn2d at every case of the dispatch table: dx against the restatement's autograd, the adjoint identity
    <upfirdn(x), dy> = <x, dx> in float64 within the two sides' bounds summed, and the second order as
    test_upfirdn2d_grads_golden forms it (d(dx . v)/d(dy) = upfirdn(v), here with v = x so that the forward's float64 result is
    the reference).  Pins _Upfirdn2d.backward's padding on odd sizes at down = 2, where in * up - out * down is not 0."""
    from brushstroke_engine_amd import ops
    case = DISPATCH[name]
    major, ih, iw, fh, fw, up, down, pad = case
    flip = list(DISPATCH).index(name) % 2 == 1
    x, f = up_inputs(case, seed=len(name) + sum(case[:5]))
    rs = np.random.RandomState(major + fh)
    dy = torch.from_numpy(rs.randn(*up_out_shape(case)).astype(np.float32))
    xr = x.double().requires_grad_(True)
    want, tol = pr.upfirdn2d_ref(xr, f, up, down, pad, flip, UP_GAIN, bound=True)
    want_dx, = torch.autograd.grad(want, [xr], dy.double())
    xa = x.double().abs().requires_grad_(True)
    s_dx, = torch.autograd.grad(pr.upfirdn2d_ref(xa, f.abs(), up, down, pad, flip, UP_GAIN), [xa], dy.double().abs())
    tol_dx = (math.ceil(fh / down[1]) * math.ceil(fw / down[0]) + 2) * U * s_dx
    want = want.detach()
    kw = dict(up=list(up), down=list(down), padding=pad, flip_filter=flip, gain=UP_GAIN)
    xd = x.to(dev)[None].requires_grad_(True)
    dyd = dy.to(dev)[None].requires_grad_(True)
    fd = f.to(dev)
    y = ops.upfirdn2d(xd, fd, **kw)
    dx, = torch.autograd.grad(y, [xd], dyd, create_graph=True)
    g, = torch.autograd.grad((dx * xd.detach()).sum(), [dyd])
    within(y[0], want, tol, f"ops.upfirdn2d {name} y")
    within(dx[0], want_dx, tol_dx, f"ops.upfirdn2d {name} dx")
    within(g[0], want, tol, f"ops.upfirdn2d {name} second order")
    lhs = float((y[0].detach().double().cpu() * dy.double()).sum())
    rhs = float((x.double() * dx[0].detach().double().cpu()).sum())
    slack = float((tol * dy.double().abs()).sum() + (tol_dx * x.double().abs()).sum())
    assert abs(lhs - rhs) <= slack, f"ops.upfirdn2d {name}: <y, dy> = {lhs!r}, <x, dx> = {rhs!r}, bound {slack:.3g}"
