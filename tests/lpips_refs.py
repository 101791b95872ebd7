"""Float64 statement of the LPIPS network (brushstroke_engine_amd/perceptual.py, csrc/nb_lpips.hip) and the cases its tests share.

No reference-made golden is possible: the ``lpips`` package is in neither tree.  The statement is written from the definition -- the
scaling layer, torchvision's ``vgg16.features`` / ``alexnet.features`` layouts with taps at ReLU outputs, and per level
``mean_hw sum_c w_c (u0_c - u1_c)^2`` with ``u = f / (sqrt(sum f^2) + 1e-10)`` -- with one convention: a pixel whose feature vector
is all zero passes no gradient through its norm.

Bounds: ``clarity_refs.bound`` (4 x the float32 torch route's error against float64 on the same inputs, plus 4 ulps of the value)."""
import numpy as np
import torch
import torch.nn.functional as F

from clarity_refs import EPS32, bound  # noqa: F401  (the project's convention, shared)

SHIFT, SCALE = (-.030, -.088, -.188), (.458, .448, .450)
VGG_CONVS, VGG_POOLS, VGG_TAPS = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28), (4, 9, 16, 23), (3, 8, 15, 22, 29)
ALEX_CONVS = {0: (11, 4, 2), 3: (5, 1, 2), 6: (3, 1, 1), 8: (3, 1, 1), 10: (3, 1, 1)}            # index: (kernel, stride, padding)
ALEX_POOLS, ALEX_TAPS = (2, 5), (1, 4, 7, 9, 11)

# Whole-network comparison with the split-f16 trunk kernels (ops.TRAIN_SPLIT_F16 = True, the default): the bound is
# SPLIT_F16_FACTOR x the float32 torch route's error plus the ulp floor.  The factor is 4 x the largest ratio
# (kernel error / float32 torch route error) MEASURED on one MI355X on the seeded cases below: vgg value 0.72, gradient 0.62; alex
# value 1.44, gradient 1.00.  The figures are the same with ops.TRAIN_SPLIT_F16 off: at these sizes (n * h * w below
# ops.TRAIN_SPLIT_F16_MIN_PIXELS) ops.conv2d sends the trunk to the fp32 kernels with either setting.
# "vgg64" (below) is the case whose two 64 x 64 layers do run the split-f16 kernels (split_up1 forward, split_up1 + tf_pack backward);
# measured there on one MI355X: value 1.77, gradient 1.00 with ops.TRAIN_SPLIT_F16 on -- within the factor, which stays as it is -- and
# value 5.93, gradient 0.69 with it off (the fp32 kernels; the value's error, 2.0e-9 against the torch route's 3.4e-10, is 0.60 of its
# bound, most of which is the ulp floor).  Measured again on the older cases: vgg 0.72 and 0.62, alex 3.11 (8.6e-10 against 2.8e-10, 0.43
# of its bound) and 0.91, with either setting.  The layer bounds of tests/test_hip_lpips_trunk_f64.py hold on every route, worst
# error / bound 0.06.
SPLIT_F16_MEASURED_RATIO = 1.44
SPLIT_F16_FACTOR = 4.0 * SPLIT_F16_MEASURED_RATIO
KINK_MARGIN = 64.0                               # pre-activations and pool gaps: this many float32-route errors away from zero

# (seeds: the first for which kink_margins holds with room -- vgg 17: 198 and 104 errors, alex 1: 900 and 306 -- found on the CPU)
SLIM = {"vgg": dict(channels=(8, 16, 24, 24, 40), size=32, n=3, seed=17), "alex": dict(channels=(8, 12, 16, 12, 12), size=64, n=2, seed=1),
        # n * h * w = 8192 = ops.TRAIN_SPLIT_F16_MIN_PIXELS at the two 64 x 64 layers; every smaller layer stays on the fp32 kernels.
        # Seed 52: 77 and 70 errors (seed 34, 94 and 64, is the only other seed below 150 that holds).  The channels are thinner than
        # "vgg"'s: (8, 16, 24, 24, 40) has no seed below 150 at this size whose margins hold (the best reaches 35 and 22 errors).
        "vgg64": dict(arch="vgg", channels=(4, 8, 12, 12, 16), size=64, n=2, seed=52)}
# the split-path branches (tests/split_branches.py) a whole-network case runs with ops.TRAIN_SPLIT_F16 on; none with it off
NETWORK_BRANCHES = {"vgg": set(), "alex": set(), "vgg64": {"split_up1", "tf_pack"}}


def layout(arch):
    """[(index, kernel, stride, padding, level or None, pool window or 0)] of the trunk's convolutions."""
    if arch == "vgg":
        return [(i, 3, 1, 1, VGG_TAPS.index(i + 1) if i + 1 in VGG_TAPS else None, 2 if i + 2 in VGG_POOLS else 0) for i in VGG_CONVS]
    return [(i, k, s, p, ALEX_TAPS.index(i + 1), 3 if i + 2 in ALEX_POOLS else 0) for i, (k, s, p) in ALEX_CONVS.items()]


def slim_weights(arch, channels, seed, size=32):
    """A seeded network of the arch's layer layout whose five levels have ``channels``; head weights mostly positive with negative
    entries.  The convolutions are normalised on a seeded probe batch of ``size`` x ``size`` images, layer by layer, so that every
    channel's pre-activation has unit spread around a bias of 2 to 3.5 spreads -- above zero for two channels of three, below it for the
    third (a channel that is mostly dead).  A random network of He-scaled weights has a tenth of a percent of its ~10^5 pre-activations
    within 64 float32-route errors of zero, whatever its seed; with the decisions spread out like this only a few elements per ten
    thousand change sign between images, and a seed whose float64 margins hold (``kink_margins``) exists."""
    rs = np.random.RandomState(seed)
    out, c_in = {"arch": np.asarray(arch)}, 3
    t64 = lambda a: torch.as_tensor(np.asarray(a, np.float64))
    x = (t64(np.tanh(rs.randn(4, 3, size, size))) - t64(SHIFT).reshape(1, 3, 1, 1)) / t64(SCALE).reshape(1, 3, 1, 1)
    level = 0
    for i, k, s, p, lvl, win in layout(arch):
        c_out = channels[level]
        w = t64(rs.randn(c_out, c_in, k, k))
        pre = F.conv2d(x, w, None, stride=s, padding=p)
        mean, std = pre.mean(dim=(0, 2, 3)), pre.std(dim=(0, 2, 3))
        sign = t64(np.where(np.arange(c_out) % 3 == 2, -1.0, 1.0))
        w32 = (w / std.reshape(-1, 1, 1, 1)).numpy().astype(np.float32)
        b32 = (-mean / std + sign * t64(rs.uniform(2.0, 3.5, c_out))).numpy().astype(np.float32)
        out[f"features.{i}.weight"], out[f"features.{i}.bias"] = w32, b32
        x = torch.relu(F.conv2d(x, t64(w32), t64(b32), stride=s, padding=p))
        if win:
            x = F.max_pool2d(x, win, 2)
        c_in = c_out
        if lvl is not None:
            lin = np.abs(rs.randn(c_out)) * 0.5
            lin[rs.rand(c_out) < 0.25] *= -0.5
            lin[0] = -abs(lin[0]) - 0.05                                   # at least one negative entry
            out[f"lin{lvl}.weight"] = lin.astype(np.float32)
            level += 1
    return out


def unit(f):
    """f / (|f| + 1e-10) over the channels; zeros, and no gradient, where |f| = 0."""
    ss = (f * f).sum(dim=1, keepdim=True)
    pos = ss > 0
    return torch.where(pos, f / (torch.sqrt(torch.where(pos, ss, torch.ones_like(ss))) + 1e-10), torch.zeros_like(f))


def head_f64(f0, f1, w):
    """[N] float64 of one level; differentiable with respect to f1."""
    f0, f1, w = (x if (torch.is_tensor(x) and x.dtype == torch.float64) else torch.as_tensor(np.asarray(x, np.float64)) for x in (f0, f1, w))
    u0, u1 = unit(f0), unit(f1)
    return ((u0 - u1) ** 2 * w.reshape(1, -1, 1, 1)).sum(dim=1).mean(dim=(1, 2))


def head_bwd_f64(f0, f1, w, g):
    """The closed form the backward kernel evaluates, numpy float64: d_f1 of sum_n g_n head_n."""
    f0, f1, w, g = (np.asarray(x, np.float64) for x in (f0, f1, w, g))
    hw = f0.shape[2] * f0.shape[3]
    wc = w.reshape(1, -1, 1, 1)
    s0, s1 = np.sqrt((f0 ** 2).sum(1, keepdims=True)), np.sqrt((f1 ** 2).sum(1, keepdims=True))
    n1 = s1 + 1e-10
    e = f1 / n1 - f0 / (s0 + 1e-10)
    q = (wc * e * f1).sum(1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        d = 2 * wc * e / n1 - f1 * 2 * q / (n1 ** 2 * s1)
    d = np.where(s1 > 0, d, 0.0)
    return d * g.reshape(-1, 1, 1, 1) / hw


def lpips_f64(weights, x0, x1, dtype=torch.float64, record=None):
    """[N] of the whole network in ``dtype`` torch operations (float64: the statement); differentiable with respect to ``x1`` when it
    is a tensor of that dtype that requires grad.  ``record``: a list that receives, per convolution of the x1 pass, (pre-activation,
    pool window)."""
    t = lambda a: a.to(dtype) if torch.is_tensor(a) else torch.as_tensor(np.asarray(a, np.float64)).to(dtype)
    arch = str(np.asarray(weights["arch"]).reshape(-1)[0])
    shift, scale = t(np.asarray(SHIFT)).reshape(1, 3, 1, 1), t(np.asarray(SCALE)).reshape(1, 3, 1, 1)

    def taps(x, rec):
        x, out = (x - shift) / scale, []
        for i, _k, s, p, lvl, win in layout(arch):
            pre = F.conv2d(x, t(weights[f"features.{i}.weight"]), t(weights[f"features.{i}.bias"]), stride=s, padding=p)
            if rec is not None:
                rec.append((pre.detach(), win))
            x = torch.relu(pre)
            if lvl is not None:
                out.append(x)
            if win:
                x = F.max_pool2d(x, win, 2)
        return out

    with torch.no_grad():
        t0 = taps(t(x0), None)
    total = 0
    for lvl, (f0, f1) in enumerate(zip(t0, taps(t(x1), record))):
        w = t(weights[f"lin{lvl}.weight"]).reshape(1, -1, 1, 1)
        u0, u1 = unit(f0), unit(f1)
        total = total + ((u0 - u1) ** 2 * w).sum(dim=1).mean(dim=(1, 2))
    return total


def kink_margins(rec64, rec32):
    """(smallest |pre-activation|, smallest gap between the two largest ReLU outputs of a pool window that holds a positive value,
    largest float32 pre-activation error) over the convolutions of a pass: a ReLU or pool decision may differ between float32 and
    float64 only where a margin is within reach of that error."""
    min_pre, min_gap, err = np.inf, np.inf, 0.0
    for (p64, win), (p32, _) in zip(rec64, rec32):
        err = max(err, float((p32.double() - p64).abs().max()))
        min_pre = min(min_pre, float(p64.abs().min()))
        if win:
            y = torch.relu(p64)
            patches = F.unfold(y.reshape(-1, 1, *y.shape[2:]), win, stride=2)                  # [N*C, win*win, L]
            top = patches.topk(2, dim=1).values
            live = top[:, 0] > 0                                               # a window of zeros passes no gradient either way
            if bool(live.any()):
                min_gap = min(min_gap, float((top[:, 0] - top[:, 1])[live].min()))
    return min_pre, min_gap, err


def network_case(name):
    """The seeded whole-network case of a name in SLIM (an arch, or a case that names its arch): weights, a target and an image in -1..1."""
    c = SLIM[name]
    arch = c.get("arch", name)
    rs = np.random.RandomState(100 + c["seed"])
    x0 = np.tanh(rs.randn(c["n"], 3, c["size"], c["size"])).astype(np.float32)
    x1 = np.clip(x0 + 0.3 * rs.randn(*x0.shape), -1, 1).astype(np.float32)
    return slim_weights(arch, c["channels"], c["seed"], c["size"]), x0, x1


HEAD_CASES = [(1, 5, 1, 1), (3, 24, 2, 2), (2, 64, 15, 15), (2, 40, 32, 32), (2, 512, 2, 2)]


def head_case(n, c, h, w, seed=0):
    """ReLU-like feature maps (non-negative, about a third zeros), a ``w`` with negative entries; where the map has at least three
    pixels: pixel 0 of sample 0 all zero in f0 only, pixel 1 in f1 only, pixel 2 in both."""
    rs = np.random.RandomState(7 * n + 11 * c + 13 * h + seed)
    f0, f1 = (np.maximum(rs.randn(n, c, h, w) + 0.4, 0).astype(np.float32) for _ in range(2))
    if h * w >= 3:
        a, b = f0.reshape(n, c, -1), f1.reshape(n, c, -1)
        a[0, :, 0] = 0
        b[0, :, 1] = 0
        a[0, :, 2] = 0
        b[0, :, 2] = 0
    wv = (np.abs(rs.randn(c)) * 0.5).astype(np.float32)
    wv[::3] *= -0.5
    g = rs.uniform(0.5, 1.5, n).astype(np.float32)
    return f0, f1, wv, g


POOL_CASES = [(1, 3, 2, 2, 2), (1, 8, 16, 16, 2), (1, 7, 15, 15, 3), (1, 5, 7, 7, 3), (1, 4, 9, 6, 0), (2, 6, 9, 9, 2), (2, 6, 9, 9, 3)]


def pool_case(n, c, h, w, seed=0):
    """Raw convolution outputs and a bias; channel 0's values are all negative after the bias."""
    rs = np.random.RandomState(1000 * c + 10 * h + w + seed)
    x, b = rs.randn(n, c, h, w).astype(np.float32), (0.3 * rs.randn(c)).astype(np.float32)
    x[:, 0] = -np.abs(x[:, 0]) - 1.0
    b[0] = -0.5
    return x, b


def pool_ref(x, b, win, dtype, d_tap=None, d_pooled=None):
    """(tap, pooled or None, d_x or None) in ``dtype`` torch on the tensors' device."""
    x = x.to(dtype).detach().requires_grad_(True)
    tap = torch.relu(x + b.to(dtype).reshape(1, -1, 1, 1))
    pooled = F.max_pool2d(tap, win, 2) if win else None
    d_x = None
    if d_tap is not None or d_pooled is not None:
        obj = 0
        if d_tap is not None:
            obj = obj + (tap * d_tap.to(dtype)).sum()
        if d_pooled is not None:
            obj = obj + (pooled * d_pooled.to(dtype)).sum()
        d_x, = torch.autograd.grad(obj, x)
    return tap.detach(), None if pooled is None else pooled.detach(), d_x


# ------------------------------------------------------------------------------------------------
# the trunk's convolutions, layer by layer, at LPIPS's own shapes (tests/test_hip_lpips_trunk_f64.py, tests/test_lpips_cpu.py)
# ------------------------------------------------------------------------------------------------
# A convolution and its input gradient are linear: no ReLU or pool decision is involved, and the bounds are the derived ones of
# tests/test_hip_train_grads_f64.py (a contraction of L terms is within (L + k + c) U S, S = the same map in float64 on |operands|;
# the split-f16 path adds the subnormal floors F_ACT and F_W).  The shapes are the smallest that still take each route of ops.conv2d /
# ops._conv2d_input_grad: n * h * w = 8192 is ops.TRAIN_SPLIT_F16_MIN_PIXELS itself.
UP1, UP1_BWD, CANVAS = {"split_up1"}, {"split_up1", "tf_pack"}, {"split_canvas"}
LAYER_CASES = [
    # id, n, ci, co, h, w, kernel, stride, padding, declared split-path branches of the forward, of the input gradient
    ("up1_3to4_64", 2, 3, 4, 64, 64, 3, 1, 1, UP1, UP1_BWD),
    ("up1_3to64_64", 2, 3, 64, 64, 64, 3, 1, 1, UP1, UP1_BWD),
    ("up1_64to64_64", 2, 64, 64, 64, 64, 3, 1, 1, UP1, UP1_BWD),
    ("up1_64to128_32", 8, 64, 128, 32, 32, 3, 1, 1, UP1, UP1_BWD),
    ("up1_12to12_16x32", 16, 12, 12, 16, 32, 3, 1, 1, UP1, UP1_BWD),
    ("control_tiled_3to64_64", 1, 3, 64, 64, 64, 3, 1, 1, set(), set()),
    ("canvas_12to16_31", 9, 12, 16, 31, 31, 3, 1, 1, CANVAS, CANVAS),          # (alex's 3x3 layers at 512 x 512 images)
    ("canvas_3to8_96", 2, 3, 8, 96, 96, 3, 1, 1, CANVAS, CANVAS),
    ("control_generic_12to16_31", 8, 12, 16, 31, 31, 3, 1, 1, set(), set()),
] + [
    # alex's first layer: image sides with remainders 0, 1, 2, 3, 0 of _conv_input_grad's right / bottom padding
    (f"alex11_3to{co}_{side}", 2, 3, co, side, side, 11, 4, 2, set(), set()) for co in (8, 64) for side in (63, 64, 65, 66, 67)
] + [
    (f"alex5_8to12_{side}", 2, 8, 12, side, side, 5, 1, 2, set(), set()) for side in (15, 7)
] + [
    (f"alex3_12to16_{side}", 2, 12, 16, side, side, 3, 1, 1, set(), set()) for side in (15, 7, 3)
]
LAYER_IDS = [c[0] for c in LAYER_CASES]
STRIDE4_REMAINDERS = {63: 0, 64: 1, 65: 2, 66: 3, 67: 0}
CATCH_FACTOR = 20.0                              # a zeroed channel must move the float64 result by this many bounds


def layer_out_size(side, k, s, p):
    return (side + 2 * p - k) // s + 1


def stride_remainder(side, k, s, p):
    """Rows (columns) of the image past the last window's reach: what perceptual._conv_input_grad pads on the right and below."""
    return side - ((layer_out_size(side, k, s, p) - 1) * s + k - 2 * p)


def layer_operands(case):
    """(x, w, d_raw) float32 of a layer case, seeded by its shape.

    x: what LPIPS feeds the layer -- the scaled image ``(tanh(randn) - shift) / scale`` where the layer has 3 input channels,
    otherwise ReLU outputs ``max(randn + 0.4, 0)`` (about a third zeros) times per-sample scales 1, 2^-6.
    d_raw: ``randn`` with three of four elements zeroed in a 2 x 2 pool pattern (one random survivor per window), times ``1 / (h w)``
    of the gradient's own map (the head's mean over pixels), times test_hip_train_grads_f64.dy_scales(n) (an all-zero sample
    where n >= 4)."""
    from test_hip_train_grads_f64 import dy_scales
    _name, n, ci, co, h, w_, k, s, p, _f, _b = case
    g = torch.Generator().manual_seed(1000 * n + 100 * ci + 10 * co + h + w_ + k)
    ho, wo = layer_out_size(h, k, s, p), layer_out_size(w_, k, s, p)
    if ci == 3:
        x = (torch.tanh(torch.randn([n, ci, h, w_], generator=g)) - torch.tensor(SHIFT).reshape(1, 3, 1, 1)) / torch.tensor(SCALE).reshape(1, 3, 1, 1)
    else:
        x = torch.clamp_min(torch.randn([n, ci, h, w_], generator=g) + 0.4, 0) * torch.tensor([[1.0, 2.0 ** -6][i % 2] for i in range(n)]).reshape(n, 1, 1, 1)
    w = torch.randn([co, ci, k, k], generator=g)
    d = torch.randn([n, co, ho, wo], generator=g)
    hh, ww = -(-ho // 2), -(-wo // 2)
    pick = torch.randint(0, 4, [n, co, hh, ww], generator=g)
    keep = F.one_hot(pick, 4).reshape(n, co, hh, ww, 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(n, co, 2 * hh, 2 * ww)[:, :, :ho, :wo]
    d = d * keep.to(d.dtype) * (1.0 / (ho * wo)) * dy_scales(n).reshape(n, 1, 1, 1)
    return x.float().contiguous(), w.float().contiguous(), d.float().contiguous()


def _vjp_x(x, w, cot, s, p):
    """d <conv2d(x, w), cot> / dx in float64."""
    x = x.detach().clone().requires_grad_(True)
    g, = torch.autograd.grad(F.conv2d(x, w, stride=s, padding=p), x, cot)
    return g


_LAYER_REFS = {}


def layer_reference(case):
    """Once per case (shared, read only): the operands, the float64 results of ``F.conv2d`` and its autograd on the same float32
    operands, the same maps on |operands| and on ones (for the bounds), and both results with channel 0 of the input (of d_raw)
    zeroed (for ``catches``)."""
    name = case[0]
    if name not in _LAYER_REFS:
        _name, n, ci, co, h, w_, k, s, p, _f, _b = case
        x, w, d = layer_operands(case)
        x64, w64, d64 = x.double(), w.double(), d.double()
        ax, aw, ad = x64.abs(), w64.abs(), d64.abs()
        conv = lambda a, b: F.conv2d(a, b, stride=s, padding=p)
        xb, db = x64.clone(), d64.clone()
        xb[:, 0] = 0
        db[:, 0] = 0
        one_w = torch.ones([co, 1, k, k], dtype=torch.float64)               # (ones for the weight: every output / input channel alike)
        _LAYER_REFS[name] = dict(
            x=x, w=w, d=d, y=conv(x64, w64), y_abs=conv(ax, aw), y_bad=conv(xb, w64),
            y_ones_x=conv(torch.ones([1, ci, h, w_], dtype=torch.float64), aw),                           # [1, co, ho, wo]
            y_ones_w=conv(ax.sum(dim=1, keepdim=True), one_w[:1]),                                        # [n, 1, ho, wo]
            dx=_vjp_x(x64, w64, d64, s, p), dx_abs=_vjp_x(ax, aw, ad, s, p), dx_bad=_vjp_x(x64, w64, db, s, p),
            dx_ones_d=_vjp_x(ax[:1], aw, torch.ones([1, co] + list(d.shape[2:]), dtype=torch.float64), s, p),   # [1, ci, h, w]
            dx_ones_w=_vjp_x(ax[:, :1], one_w, ad, s, p),                                                 # [n, 1, h, w]
            max_x=float(ax.max()), max_d=float(ad.max()))
    return _LAYER_REFS[name]


def layer_bounds(case, ref, split):
    """Element bounds (t_y, t_dx) of a layer case.  ``split``: the case runs on the split-f16 kernels (its declared branches are not
    empty and ops.TRAIN_SPLIT_F16 is on) -- the fp32 kernels get the fp32 bound in either mode.

    y:  (k k ci + 36 + cs) U S, S = conv(|x|, |w|); split: + F_ACT max|x| conv(1, |w|) + F_W conv(|x|, 1).
    dx: test_conv_grads_vs_float64's t_dx with L = k k co (the stuffed stride-4 backward: 121 co, the stuffed zeros add exact zeros):
        (L + 16 + 20 + cs) U S, S = the gradient's map on |d_raw|, |w|; split: + F_ACT max|d_raw| map(1, |w|) + F_W map(|d_raw|, 1)."""
    from test_hip_train_grads_f64 import C_SPLIT, F_ACT, F_W, U
    _name, _n, ci, co, _h, _w, k, _s, _p, _f, _b = case
    cs = C_SPLIT if split else 0
    t_y = (k * k * ci + 36 + cs) * U * ref["y_abs"]
    t_dx = (k * k * co + 16 + 20 + cs) * U * ref["dx_abs"]
    if split:
        t_y = t_y + F_ACT * ref["max_x"] * ref["y_ones_x"] + F_W * ref["y_ones_w"]
        t_dx = t_dx + F_ACT * ref["max_d"] * ref["dx_ones_d"] + F_W * ref["dx_ones_w"]
    return t_y, t_dx
