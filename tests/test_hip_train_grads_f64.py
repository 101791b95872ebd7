"""GPU: first- and second-order gradients of the training path's differentiable operators (ops.modulated_conv2d, ops.conv2d,
ops.conv2d_down2) at the sizes where they run on the split-f16 kernels, and on the exact-fp32 kernels (TRAIN_SPLIT_F16 =
WGRAD_SPLIT_F16 = False), against float64 autograd on the CPU (oracle.conv2d_resample / upfirdn2d).

Every case declares the split-path branches it exists for; the wrappers of tests/split_branches.py (around ops._conv2d_launch,
ops._split_f16_eligible, ops._conv2d_s2_valid_h3, ops._s2_valid_h3_supported, ops.pack_conv_weight_h3_dev and the split
weight-gradient entry) record the branches that ran, and the two sets must agree (no split-path branch at all on the exact-fp32
path), so a moved threshold cannot take a case off its path unnoticed.

Bounds (tests/test_hip_train_kernels.py): a contraction of L terms is within (L + k + c) U S, S = the float64 sum of |terms|
-- obtained by running the same linear map on |operands| -- with c = 14 per split-f16 product (0 on the fp32 kernels).  The
split path adds subnormal floors: range-packed activations (scale k with max|a| k in (2^13, 2^14]) lose <= 2^-24 / k <= 2^-37
max|a| per element, weights (packed unscaled) <= 2^-25, weight-gradient operands (max near 2^10) <= 2^-33 max|.|; each floor
times the sum of the other operand's |terms| (the map run with ones in place of the floored operand).  The composites of
modulated_conv2d (dW, ds from dd and dq; _ModulatedConv2d docstring) carry their inputs' bounds through that formula.  Each
case also shows its bounds can catch an error: zeroing one input channel (and one dy channel) in the float64 reference must
move every checked gradient by >= 20x its largest bound.  The modulated-convolution inputs have a non-zero mean: with zero-mean
operands ds and the path-length gradient would be random-signed sums of ~sqrt(L) |term| against bounds of ~L U sum|terms|."""
import pytest
import torch

import split_branches
from brushstroke_engine_amd import ops
from oracle import neube_oracle as orc
from test_hip_step_kernels import U, within

pytestmark = pytest.mark.gpu
C_SPLIT = 14
F_ACT, F_W, F_WG = 2.0 ** -37, 2.0 ** -25, 2.0 ** -33
SPLIT_TOKENS = split_branches.SPLIT_TOKENS
FIR = orc.setup_filter(dtype=torch.float64)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


@pytest.fixture(params=[True, False], ids=["split_f16", "fp32"])
def mode(request, monkeypatch):
    """Sets TRAIN_SPLIT_F16 = WGRAD_SPLIT_F16 and records the split-path branches that run (tests/split_branches.py); flags restored
    on the way out."""
    split = request.param
    rec = split_branches.record(monkeypatch)
    with split_branches.flags(split):
        yield split, rec


def branches_ok(mode, declared, what):
    """Split mode: the branches that ran are the declared ones plus the split weight-gradient kernel (WGRAD_SPLIT_F16 holds at
    every size; every case here computes a weight gradient).  fp32 mode: no split-path branch at all."""
    split, rec = mode
    split_branches.check(split, rec, set(declared) | {"wgrad_h3"}, what)


def vjp(fn, args, i, cot):
    """d<fn(args), cot>/d args[i] in float64."""
    args = [a.detach().clone().requires_grad_(j == i) for j, a in enumerate(args)]
    g, = torch.autograd.grad(fn(*args), args[i], cot)
    return g


def catches(want, bad, tol, what):
    moved, t = float((want - bad).abs().max()), float(tol.max())
    assert moved >= 20 * t, f"{what}: a zeroed input channel moves it by {moved:.3g}, bound {t:.3g}: the check is blind"


def gen(seed, *shapes):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=g) for s in shapes]


def dy_scales(n):
    """Per-sample scales of dy: 1, 2^-6, 2^-12 and one all-zero sample (range scale is one power of two per tensor)."""
    return torch.tensor([[1.0, 2.0 ** -6, 2.0 ** -12, 0.0][i % 4] if n >= 4 else [1.0, 2.0 ** -12][i % 2] for i in range(n)])


# ---------------------------------------------------------------------------------------------------------------------
# modulated_conv2d
# ---------------------------------------------------------------------------------------------------------------------

def lin(x, w, s, up):
    return orc.conv2d_resample(x * s[:, :, None, None], w, f=FIR, up=up, padding=1, flip_weight=(up == 1))


def demod(s, w):
    return (s.square() @ w.square().sum(dim=[2, 3]).t() + 1e-8).rsqrt()


def modconv_ref(x, w, s, nz, dy, up):
    """float64 gradients (dx, dw, ds, dnoise) of y = lin(x, w, s) d + noise."""
    x, w, s, nz = [t.detach().clone().requires_grad_(True) for t in (x, w, s, nz)]
    y = lin(x, w, s, up) * demod(s, w)[:, :, None, None] + nz
    return y.detach(), torch.autograd.grad(y, [x, w, s, nz], dy)


def modconv_bounds(x, w, s, nz, dy, y, up, split):
    """Element bounds of (dx, dw, ds, dnoise), carried through dd = sum dy (y - noise), dq = -1/2 d^2 dd,
    dW = sum_n s A + 2 W sum_n dq s^2, ds = sum_{o,t} W A + 2 s sum_o dq Wsq."""
    n, c, h, wd = x.shape
    o = w.shape[0]
    cs = C_SPLIT if split else 0
    d = demod(s, w)
    dd4 = d[:, :, None, None]
    ax, aw, as_, ady = x.abs(), w.abs(), s.abs(), dy.abs()
    one_x, one_w = torch.ones_like(x), torch.ones_like(w)
    fir = 4 if up == 2 else 1                                      # the up = 2 kernels fold the 4x4 FIR into the products
    ed = (c + 8) * U                                               # relative error of d (fp32 s^2 @ Wsq, rsqrt)
    # forward y: 9 c fir products; the noise add; d
    e_fwd = (9 * c * fir + 16 + cs) * U + ed
    y_abs = lin(ax, aw, as_, up) * dd4
    t_y = e_fwd * y_abs + U * y.abs()
    if split:
        t_y = t_y + fir * dd4 * (F_ACT * float((x * s[:, :, None, None]).abs().max()) * lin(one_x, aw, torch.ones_like(s), up)
                                 + F_W * lin(ax, one_w, as_, up))
    # dx = s corr(dy d, W^T)
    e_dx = (9 * o * fir + 16 + 20 + cs) * U + ed
    adz = ady * dd4
    t_dx = e_dx * vjp(lambda a: lin(a, aw, as_, up), [ax], 0, adz)
    if split:
        mz = float((dy * dd4).abs().max()) * 4
        t_dx = t_dx + fir * (F_ACT * mz * vjp(lambda a: lin(a, aw, as_, up), [ax], 0, torch.ones_like(dy))
                             + F_W * vjp(lambda a: lin(a, one_w, as_, up), [ax], 0, adz))
    # A (per-sample weight-gradient correlation): hw (up = 1) or (2h + 1)^2 (up = 2, on the FIR adjoint of dz) products
    la = h * wd if up == 1 else (2 * h + 1) * (2 * wd + 1)
    e_a = (la + n + 16 + (20 if up == 2 else 0) + cs) * U + ed
    dwd_abs = vjp(lambda b: lin(ax, b, as_, up), [aw], 0, adz)
    dsd_abs = vjp(lambda b: lin(ax, aw, b, up), [as_], 0, adz)
    t_dwd, t_dsd = e_a * dwd_abs, e_a * dsd_abs
    if split:
        mx, mz = float(x.abs().max()), float((dy * dd4).abs().max()) * 4
        t_dwd = t_dwd + F_WG * (mx * vjp(lambda b: lin(one_x, b, as_, up), [aw], 0, adz) + mz * vjp(lambda b: lin(ax, b, as_, up), [aw], 0, torch.ones_like(dy)))
        t_dsd = t_dsd + F_WG * (mx * vjp(lambda b: lin(one_x, aw, b, up), [as_], 0, adz) + mz * vjp(lambda b: lin(ax, aw, b, up), [as_], 0, torch.ones_like(dy)))
    # dd, dq
    ymn = (y - nz).abs()
    t_dd = (h * wd * fir + 4) * U * (ady * ymn).sum(dim=[2, 3]) + (ady * t_y).sum(dim=[2, 3])
    dd = (dy * (y - nz)).sum(dim=[2, 3])
    dq = -0.5 * d.square() * dd
    t_dq = 0.5 * d.square() * t_dd + (2 * ed + 3 * U) * dq.abs()
    wsq = w.square().sum(dim=[2, 3])                               # [o, c]
    s2 = s.square()
    t_dw = t_dwd + (n + 6) * U * (dwd_abs + 2 * aw * (dq.abs().t() @ s2)[:, :, None, None]) + 2 * aw * (t_dq.t() @ s2)[:, :, None, None]
    t_ds = t_dsd + (9 * o + 14) * U * (dsd_abs + 2 * as_ * (dq.abs() @ wsq)) + 2 * as_ * (t_dq @ wsq)
    t_dn = (o + 2) * U * ady.sum(dim=1, keepdim=True)
    return t_dx, t_dw, t_ds, t_dn


MODCONV_CASES = [
    # id, up, n, c, o, h, noise gain, declared split-path branches
    ("up1_36to40", 1, 2, 36, 40, 64, 1.0, {"split_up1", "tf_pack"}),
    ("up1_noise100", 1, 2, 36, 40, 64, 100.0, {"split_up1", "tf_pack"}),
    ("up1_w128", 1, 8, 128, 128, 32, 1.0, {"split_up1", "tf_pack"}),
    ("up1_control", 1, 2, 36, 40, 32, 1.0, set()),
    ("up2_w32_dx_generic", 2, 2, 36, 40, 32, 1.0, {"split_up2_w32", "s2_generic"}),
    ("up2_w32_dx_s2wide", 2, 4, 36, 40, 32, 1.0, {"split_up2_w32", "s2v_wide"}),
    ("up2_w16_dx_s2narrow", 2, 16, 36, 40, 16, 1.0, {"split_up2_w16", "s2v_narrow"}),
    ("up2_control", 2, 2, 36, 40, 16, 1.0, {"s2_generic"}),
]


@pytest.mark.parametrize("case", MODCONV_CASES, ids=[c[0] for c in MODCONV_CASES])
def test_modulated_conv2d_grads_vs_float64(dev, mode, case):
    """dx, dW, ds, dnoise of ops.modulated_conv2d (demodulated, per-sample noise) against float64 autograd: per-sample dy
    scales 1 / 2^-6 / 2^-12 / 0 (each sample against its own bound), noise up to 100x the conv output (dd is formed from
    y - noise: the bound carries U sum|dy| |noise| through t_y), and an all-zero dy (exact zeros)."""
    name, up, n, c, o, h, ngain, declared = case
    split = mode[0]
    x, w, s, nz, dy = gen(n * c + h + up, [n, c, h, h], [o, c, 3, 3], [n, c], [n, 1, h * up, h * up], [n, o, h * up, h * up])
    x, nz = x + 1, nz * ngain                        # (x, dy offset: a coherent A = sum_pix x dz, so ds is not a random-signed sum)
    dy = (dy + 1) * dy_scales(n)[:, None, None, None]
    f = orc.setup_filter().to(dev)
    xd, wd_, sd, nd = [t.to(dev).requires_grad_(True) for t in (x, w, s, nz)]
    yd = ops.modulated_conv2d(xd, wd_, sd, noise=nd, up=up, padding=1, resample_filter=f if up == 2 else None, flip_weight=(up == 1))
    got = torch.autograd.grad(yd, [xd, wd_, sd, nd], dy.to(dev))
    torch.cuda.synchronize()
    branches_ok(mode, declared, name)
    x64, w64, s64, n64, dy64 = [t.double() for t in (x, w, s, nz, dy)]
    y64, want = modconv_ref(x64, w64, s64, n64, dy64, up)
    tols = modconv_bounds(x64, w64, s64, n64, dy64, y64, up, split)
    xb, dyb = x64.clone(), dy64.clone()
    xb[:, 0] = 0
    dyb[:, 0] = 0
    _, bad = modconv_ref(xb, w64, s64, n64, dyb, up)
    for nm, g, wt, t, b in zip(("dx", "dw", "ds", "dnoise"), got, want, tols, bad):
        catches(wt, b, t, f"{name} {nm}")
        within(g, wt, t, f"{name} {'split' if split else 'fp32'} {nm}")
    # an all-zero dy gives exact zeros
    yd = ops.modulated_conv2d(xd, wd_, sd, noise=nd, up=up, padding=1, resample_filter=f if up == 2 else None, flip_weight=(up == 1))
    zero = torch.autograd.grad(yd, [xd, wd_, sd, nd], torch.zeros_like(yd))
    for nm, g in zip(("dx", "dw", "ds", "dnoise"), zero):
        assert not torch.isnan(g).any() and float(g.abs().max()) == 0.0, f"{name}: all-zero dy gives {nm} {float(g.abs().max())}"


# ---------------------------------------------------------------------------------------------------------------------
# conv2d (3x3 / 1x1, odd-size embedded correlation) and conv2d_down2
# ---------------------------------------------------------------------------------------------------------------------

def down2(x, w):
    return torch.nn.functional.conv2d(orc.upfirdn2d(x, FIR, padding=(2, 2, 2, 2)), w, stride=2)


CONV_CASES = [
    # id, op, n, c, o, h, k, padding, declared split-path branches
    ("c3_pow2_fastpath", "conv", 2, 36, 40, 64, 3, 1, {"split_up1", "tf_pack"}),
    ("c3_control", "conv", 2, 36, 40, 32, 3, 1, set()),
    ("c1_centre_tap", "conv", 2, 36, 40, 64, 1, 0, set()),
    ("odd_pad0", "conv", 5, 24, 40, 45, 3, 0, {"split_canvas"}),
    ("odd_pad1", "conv", 5, 24, 40, 45, 3, 1, {"split_canvas"}),
    ("odd_pad2", "conv", 5, 24, 40, 45, 3, 2, {"split_canvas"}),
    ("odd_control", "conv", 2, 24, 40, 23, 3, 1, set()),
    ("down2_wide", "down2", 4, 24, 40, 64, 3, 0, {"s2v_wide", "split_up2_w32"}),
    ("down2_narrow", "down2", 16, 24, 40, 32, 3, 0, {"s2v_narrow", "split_up2_w16"}),
    ("down2_control", "down2", 2, 24, 40, 32, 3, 0, {"s2_generic"}),
]


@pytest.mark.parametrize("case", CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_conv_grads_vs_float64(dev, mode, case):
    """dx and dw of ops.conv2d (pow2 3x3 through the first-order fast path, 1x1 as the centre tap of the 3x3 weight gradient,
    odd sizes embedded in a tileable canvas at padding 0 / 1 / 2) and of ops.conv2d_down2 (dx through the fused up=2 kernel,
    forward through nb_conv3x3_s2_valid_h3) against float64 autograd; dy per-sample scales as above."""
    name, op, n, c, o, h, k, pad, declared = case
    split = mode[0]
    cs = C_SPLIT if split else 0
    fn = (lambda a, b: torch.nn.functional.conv2d(a, b, padding=pad)) if op == "conv" else down2
    ho = (h + 2 * pad - k + 1) if op == "conv" else h // 2
    x, w, dy = gen(n * c + h + pad + k, [n, c, h, h], [o, c, k, k], [n, o, ho, ho])
    dy = dy * dy_scales(n)[:, None, None, None]
    f = orc.setup_filter().to(dev)
    xd, wd_ = x.to(dev).requires_grad_(True), w.to(dev).requires_grad_(True)
    yd = ops.conv2d(xd, wd_, stride=1, padding=pad) if op == "conv" else ops.conv2d_down2(xd, wd_, f)
    got = torch.autograd.grad(yd, [xd, wd_], dy.to(dev))
    torch.cuda.synchronize()
    branches_ok(mode, declared, name)
    x64, w64, dy64 = x.double(), w.double(), dy.double()
    want = [vjp(fn, [x64, w64], i, dy64) for i in (0, 1)]
    ax, aw, ady = x64.abs(), w64.abs(), dy64.abs()
    fir = 4 if op == "down2" else 1
    t_dx = (k * k * o * fir + 16 + 20 + cs) * U * vjp(fn, [ax, aw], 0, ady)
    t_dw = (n * ho * ho + 16 + 20 + cs) * U * vjp(fn, [ax, aw], 1, ady)
    if split:
        mdy, mx = float(dy.abs().max()), float(x.abs().max())
        t_dx = t_dx + fir * (F_ACT * mdy * vjp(fn, [ax, aw], 0, torch.ones_like(dy64)) + F_W * vjp(fn, [ax, torch.ones_like(w64)], 0, ady))
        t_dw = t_dw + F_WG * (mx * vjp(fn, [torch.ones_like(x64), aw], 1, ady) + mdy * vjp(fn, [ax, aw], 1, torch.ones_like(dy64)))
    xb, dyb = x64.clone(), dy64.clone()
    xb[:, 0] = 0
    dyb[:, 0] = 0
    for i, (nm, t) in enumerate((("dx", t_dx), ("dw", t_dw))):
        catches(want[i], vjp(fn, [xb, w64], i, dyb), t, f"{name} {nm}")
        within(got[i], want[i], t, f"{name} {'split' if split else 'fp32'} {nm}")


# ---------------------------------------------------------------------------------------------------------------------
# create_graph: R1-type d/dw |dy/dx|^2 and path-length-type d/dw |d(y r)/ds|^2
# ---------------------------------------------------------------------------------------------------------------------

SECOND_CASES = [
    # id, op, n, c, o, h, declared split-path branches
    ("r1_conv", "conv", 2, 24, 32, 64, {"split_up1"}),
    ("r1_down2", "down2", 4, 24, 32, 64, {"s2v_wide", "split_canvas"}),
    ("pl_modconv", "modconv", 2, 36, 40, 64, {"split_up1"}),
    ("pl_control", "modconv", 2, 36, 40, 32, set()),
]


@pytest.mark.parametrize("case", SECOND_CASES, ids=[c[0] for c in SECOND_CASES])
def test_second_order_grads_vs_float64(dev, mode, case):
    """Gradients of gradients (create_graph=True): R1-type pen = |d(y . r)/dx|^2 through conv2d / conv2d_down2, path-length-type
    pen = |d(y . r)/ds|^2 through modulated_conv2d (demodulate=False: a polynomial, so the float64 run on |operands| is the sum
    of |terms|), d pen / dw against float64 autograd.  Bound: the first gradient's contraction (9 o fir) and the weight-gradient
    contraction (n ho wo) in series, twice the split-product term: (L1 + L2 + 48 + 2 c) U S."""
    name, op, n, c, o, h, declared = case
    split = mode[0]
    cs = C_SPLIT if split else 0
    ho = h // 2 if op == "down2" else h
    x, w, s, r = gen(n * c + h, [n, c, h, h], [o, c, 3, 3], [n, c], [n, o, ho, ho])
    if op == "modconv":
        x, r = x + 1, r + 1                          # (d/ds sums over the whole image: coherent operands keep S near |value|)
    f = orc.setup_filter().to(dev)

    def pen(fwd, a, b, sv, rr):
        y = fwd(a, b, sv)
        g, = torch.autograd.grad((y * rr).sum(), [sv if op == "modconv" else a], create_graph=True)
        return g.square().sum()

    if op == "modconv":
        hip = lambda a, b, sv: ops.modulated_conv2d(a, b, sv, up=1, padding=1, demodulate=False)
        ref = lambda a, b, sv: lin(a, b, sv, 1)
    elif op == "conv":
        hip = lambda a, b, sv: ops.conv2d(a, b, stride=1, padding=1)
        ref = lambda a, b, sv: torch.nn.functional.conv2d(a, b, padding=1)
    else:
        hip = lambda a, b, sv: ops.conv2d_down2(a, b, f)
        ref = lambda a, b, sv: down2(a, b)
    xd, wd_, sd = x.to(dev).requires_grad_(True), w.to(dev).requires_grad_(True), s.to(dev).requires_grad_(True)
    got, = torch.autograd.grad(pen(hip, xd, wd_, sd, r.to(dev)), [wd_])
    torch.cuda.synchronize()
    branches_ok(mode, declared, name)

    def ref_grad(a, b, sv, rr):
        a, b, sv = [t.detach().clone().requires_grad_(True) for t in (a, b, sv)]
        g, = torch.autograd.grad(pen(ref, a, b, sv, rr), [b])
        return g

    x64, w64, s64, r64 = x.double(), w.double(), s.double(), r.double()
    want = ref_grad(x64, w64, s64, r64)
    S = ref_grad(x64.abs(), w64.abs(), s64.abs(), r64.abs())
    fir = 4 if op == "down2" else 1
    l1 = 9 * o * fir if op != "modconv" else h * h                         # (d/ds: a per-sample sum over the image)
    tol = (l1 + n * ho * ho + 48 + 2 * cs) * U * S
    xb, rb = x64.clone(), r64.clone()
    xb[:, 0] = 0
    rb[:, 0] = 0
    catches(want, ref_grad(xb, w64, s64, rb), tol, name)
    within(got, want, tol, f"{name} {'split' if split else 'fp32'}")


# ---------------------------------------------------------------------------------------------------------------------
# model level: TrainableGenerator at R = 128 against OracleGenerator(float64)
# ---------------------------------------------------------------------------------------------------------------------

def _gen_setup(n=4, seed=5):
    """R = 128 at channel_max 64: the 64^2 / 128^2 layers (up = 1 and up = 2) take the split path, the 4^2 .. 16^2 ones do not."""
    import numpy as np
    from brushstroke_engine_amd import config as cfgmod, weights as wmod, synthetic
    cfg = cfgmod.GeneratorConfig(z_dim=32, w_dim=32, img_resolution=128, channel_base=128 * 16, channel_max=64, geom_feature_channels=(4, 8))
    sd = wmod.random_state_dict(cfg, seed)
    z = synthetic.batch_z(cfg, n, 3).astype(np.float32)
    geom = [g.astype(np.float32) for g in synthetic.geom_features(cfg, n, 7)]
    return cfg, sd, z, geom, synthetic.positions(cfg, n, 9)


def test_generator_gmain_grads_r128_vs_float64(dev, mode):
    """Gmain-type gradients (every parameter and z) of TrainableGenerator at R = 128, n = 4 against OracleGenerator(float64):
    2e-4 of each gradient's scale (test_trainable_gradients_match_oracle's bound).

    The geometry features' gradients are not compared here (they are at R = 32, to 2e-4, by that test).  At this size they
    are not a continuous function of the forward values within fp32 rounding: some of the ~10^6 leaky-ReLU pre-activations lie
    within the forward rounding of 0, and which slope such an element takes moves these small gradients (scale ~5e-5, a sum that
    cancels almost completely) locally.  In float64, scaling z by (1 + 1e-6 eps), eps ~ N(0, 1) per element, moves geom1's gradient by 2e-6 of its scale,
    by (1 + 1e-5 eps) by 1e-2 of its scale.  The HIP path misses 2e-4 by 2.2x on geom1 (1.6e-4 on geom0), with the whole
    deviation in one sample and three rows, identical on the split-f16 and the fp32 kernels; a plain fp32 evaluation of the
    oracle misses it by 9x / 33x."""
    import numpy as np
    from brushstroke_engine_amd.training import TrainableGenerator
    cfg, sd, z, geom, pos = _gen_setup()
    rs = np.random.RandomState(1)
    target = rs.randn(z.shape[0], 3, cfg.img_resolution, cfg.img_resolution).astype(np.float32)   # (both sides see the same fp32 inputs)
    npos = ((pos % cfg.img_resolution) / (cfg.img_resolution - 1)).astype(np.float32)
    T = TrainableGenerator(cfg, sd, dev)
    zt = torch.tensor(z, device=dev, requires_grad=True)
    gt = [torch.tensor(g, device=dev, requires_grad=True) for g in geom]
    img_t = T(zt, None, gt, positions=torch.from_numpy(pos).to(dev), noise_mode="const")
    loss_t = ((img_t - torch.from_numpy(target).to(dev)) ** 2).mean()
    O = orc.OracleGenerator(cfg, sd, dtype=torch.float64)
    keys = [k for k in O.sd if k.endswith((".weight", ".bias", ".noise_strength", ".const", ".color_bias"))]
    params = dict(T.named_reference_parameters())
    grads_t = torch.autograd.grad(loss_t, [params[k] for k in keys] + [zt], allow_unused=True)
    torch.cuda.synchronize()
    split, rec = mode
    if split:
        assert {"split_up1", "split_up2_w32", "wgrad_h3", "off_split"} <= rec, f"the R = 128 layers did not take (and leave) the split path: {sorted(rec)}"
    branches_ok(mode, rec - {"off_split"} if split else set(), "generator")
    for k in keys:
        O.sd[k].requires_grad_(True)
    zo = torch.tensor(z, dtype=torch.float64, requires_grad=True)
    go = [torch.tensor(g, dtype=torch.float64, requires_grad=True) for g in geom]
    img_o, _ = O.synthesis(O.mapping(zo), go, return_debug_data=True, norm_noise_positions=npos)
    loss_o = ((img_o - torch.from_numpy(target).double()) ** 2).mean()
    assert abs(float(loss_t.detach()) - float(loss_o.detach())) <= 1e-5 * max(1.0, abs(float(loss_o.detach())))
    grads_o = torch.autograd.grad(loss_o, [O.sd[k] for k in keys] + [zo], allow_unused=True)
    checked = 0
    for name, a, b in zip(keys + ["z"], grads_t, grads_o):
        if b is None:
            assert a is None or float(a.abs().max()) == 0.0, name
            continue
        scale = max(float(b.abs().max()), 1e-8)
        err = float((a.cpu().double() - b).abs().max())
        assert err <= 2e-4 * scale + 1e-9, (name, err, scale)
        checked += 1
    assert checked >= len(keys) - 2


def test_generator_greg_r128_vs_float64(dev, mode):
    """Greg (path length) of TrainableGenerator at R = 128, n = 4 against OracleGenerator(float64): 2e-2 of each gradient's scale
    (test_path_length_regulariser_matches_oracle's bound)."""
    import numpy as np
    from brushstroke_engine_amd.training import TrainableGenerator, TrainableDiscriminator, GanLoss, random_discriminator_state_dict
    cfg, sd, z, geom, pos = _gen_setup()
    rs = np.random.RandomState(2)
    b = 2
    noise = (rs.randn(b, 3, cfg.img_resolution, cfg.img_resolution) / cfg.img_resolution).astype(np.float32)
    G = TrainableGenerator(cfg, sd, dev)
    D = TrainableDiscriminator(random_discriminator_state_dict(32, 3, channel_base=512, channel_max=24), 32, 3, channel_base=512,
                               channel_max=24, device=dev)
    loss = GanLoss(G, D, style_mixing_prob=0, noise_mode="const")
    st = loss.accumulate_gradients("Greg", None, [torch.from_numpy(g).to(dev) for g in geom], torch.from_numpy(z).to(dev),
                                   pl_noise=torch.from_numpy(noise).to(dev))
    torch.cuda.synchronize()
    split, rec = mode
    if split:
        assert {"split_up1", "split_up2_w32", "wgrad_h3", "off_split"} <= rec, f"the R = 128 layers did not take (and leave) the split path: {sorted(rec)}"
    branches_ok(mode, rec - {"off_split"} if split else set(), "generator greg")
    O = orc.OracleGenerator(cfg, sd, dtype=torch.float64)
    keys = [k for k in O.sd if k.endswith((".weight", ".bias", ".noise_strength", ".const", ".color_bias"))]
    for k in keys:
        O.sd[k].requires_grad_(True)
    ws = O.mapping(torch.tensor(z[:b], dtype=torch.float64))
    img, _ = O.synthesis(ws, [torch.tensor(g[:b], dtype=torch.float64) for g in geom], return_debug_data=True)
    plg, = torch.autograd.grad((img * torch.tensor(noise, dtype=torch.float64)).sum(), [ws], create_graph=True)
    pl_len = plg.square().sum(2).mean(1).sqrt()
    pl_mean = torch.zeros([], dtype=torch.float64).lerp(pl_len.mean(), 0.01).detach()
    grads_o = torch.autograd.grad(((pl_len - pl_mean).square() * 2.0).mean(), [O.sd[k] for k in keys], allow_unused=True)
    want_pen = float((pl_len - pl_mean).square().mean().detach())
    assert abs(st["Loss/pl_penalty"] - want_pen) <= 1e-3 * want_pen
    params = dict(G.named_reference_parameters())
    checked = 0
    for k, go in zip(keys, grads_o):
        gt = params[k].grad
        if go is None or float(go.abs().max()) == 0.0:
            assert gt is None or float(gt.abs().max()) <= 1e-7
            continue
        scale = float(go.abs().max())
        err = float((gt.cpu().double() - go).abs().max())
        assert err <= 2e-2 * scale + 1e-9, (k, err, scale)
        checked += 1
    assert checked >= 20
