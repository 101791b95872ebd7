"""GPU: the LPIPS kernels (csrc/nb_lpips.hip) against the float64 statement of tests/lpips_refs.py at the smallest shapes that can go
wrong, the whole network on routes "hip", "torch" and float64, and the wiring into the projector and the clarity optimiser.

Bound of every summed quantity (clarity_refs.bound): 4 x the error of the float32 torch route on the same inputs against float64 plus
4 float32 ulps of the value.  Outputs sit between sentinel guards, two launches give the same bytes, and sample n of an N-sample
launch is the one-sample launch on it."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import clarity_refs as cr
import lpips_refs as lr
import projection_refs as pr
import split_branches
from brushstroke_engine_amd import _lib, clarity, config as cfgmod, ops, perceptual, projection, weights as wmod

pytestmark = pytest.mark.gpu
GUARD = 64
DEV = "cuda"


class Guarded:
    """A device buffer of ``numel`` floats between two guards of a sentinel value; ``intact()`` after the launches."""

    def __init__(self, numel, sentinel=777.0, guard=GUARD):
        self.buf = torch.full([numel + 2 * guard], sentinel, dtype=torch.float32, device=DEV)
        self.view, self.guard, self.sentinel = self.buf[guard:guard + numel], guard, sentinel

    def intact(self):
        return bool((self.buf[:self.guard] == self.sentinel).all()) and bool((self.buf[-self.guard:] == self.sentinel).all())


def _st():
    return torch.cuda.current_stream().cuda_stream


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _within(got, want, bnd, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err = np.abs(got - want)
    worst = int(np.argmax(err - bnd))
    print(f"[lpips] {what}: max err {err.max():.3g}, smallest bound {np.min(bnd):.3g}, worst err/bound {(err / np.maximum(bnd, 1e-300)).max():.3g}")
    assert np.all(np.isfinite(got)) and np.all(err <= bnd), (what, err.reshape(-1)[worst], np.broadcast_to(bnd, err.shape).reshape(-1)[worst])


# ------------------------------------------------------------------------------------------------
# scaling layer
# ------------------------------------------------------------------------------------------------
def _launch_scale(x, shift, scale):
    n, c, h, w = x.shape
    y = Guarded(x.numel())
    _lib.check(_lib.lib().nb_lpips_scale_f32(x.data_ptr(), None if shift is None else shift.data_ptr(), scale.data_ptr(), y.view.data_ptr(), n, c, h * w,
                                             _st()), "lpips_scale")
    torch.cuda.synchronize()
    assert y.intact()
    return y.view.view(n, c, h, w).cpu().numpy()


def test_scale_entry():
    rs = np.random.RandomState(0)
    x = np.tanh(rs.randn(2, 3, 5, 3)).astype(np.float32)
    shift, scale = np.asarray(lr.SHIFT, np.float32), np.asarray(lr.SCALE, np.float32)
    xd, sh, sc = _dev(x), _dev(shift), _dev(scale)
    got = _launch_scale(xd, sh, sc)
    assert got.tobytes() == _launch_scale(xd, sh, sc).tobytes()
    want = (x.astype(np.float64) - shift.astype(np.float64).reshape(1, 3, 1, 1)) / scale.astype(np.float64).reshape(1, 3, 1, 1)
    t32 = ((xd - sh.reshape(1, 3, 1, 1)) / sc.reshape(1, 3, 1, 1)).cpu().numpy()
    _within(got, want, cr.bound(t32, want), "scale")
    back = _launch_scale(xd, None, sc)                                     # the backward: no shift
    want = x.astype(np.float64) / scale.astype(np.float64).reshape(1, 3, 1, 1)
    _within(back, want, cr.bound((xd / sc.reshape(1, 3, 1, 1)).cpu().numpy(), want), "scale backward")
    assert _launch_scale(xd[1:], sh, sc).tobytes() == got[1:].tobytes()


# ------------------------------------------------------------------------------------------------
# bias + ReLU + tap + pool
# ------------------------------------------------------------------------------------------------
def _pool_shape(h, w, win):
    return ((h - win) // 2 + 1, (w - win) // 2 + 1) if win else (0, 0)


def _launch_pool(x, b, win):
    n, c, h, w = x.shape
    ph, pw = _pool_shape(h, w, win)
    tap, pooled = Guarded(x.numel()), Guarded(n * c * ph * pw)
    _lib.check(_lib.lib().nb_lpips_relu_pool_f32(x.data_ptr(), b.data_ptr(), tap.view.data_ptr(), pooled.view.data_ptr() if win else None, n, c, h, w,
                                                 win, _st()), "lpips_relu_pool")
    torch.cuda.synchronize()
    assert tap.intact() and pooled.intact()
    return tap.view.view(n, c, h, w), pooled.view.view(n, c, ph, pw)


def _launch_pool_bwd(tap, d_tap, d_pooled, win):
    n, c, h, w = tap.shape
    d_x = Guarded(tap.numel())
    _lib.check(_lib.lib().nb_lpips_relu_pool_bwd_f32(tap.data_ptr(), None if d_tap is None else d_tap.data_ptr(),
                                                     None if d_pooled is None else d_pooled.data_ptr(), d_x.view.data_ptr(), n, c, h, w, win, _st()),
               "lpips_relu_pool_bwd")
    torch.cuda.synchronize()
    assert d_x.intact()
    return d_x.view.view(n, c, h, w).cpu().numpy()


@pytest.mark.parametrize("n,c,h,w,win", lr.POOL_CASES, ids=[f"n{n}_c{c}_{h}x{w}_win{win}" for n, c, h, w, win in lr.POOL_CASES])
def test_relu_pool_entries(n, c, h, w, win):
    x, b = lr.pool_case(n, c, h, w)
    xd, bd = _dev(x), _dev(b)
    tap, pooled = _launch_pool(xd, bd, win)
    tap2, pooled2 = _launch_pool(xd, bd, win)
    assert torch.equal(tap, tap2) and torch.equal(pooled, pooled2)
    # forward: one add and maxima, each exactly rounded -- the bytes of float32 torch on the device
    t_tap, t_pooled, _ = lr.pool_ref(xd, bd, win, torch.float32)
    assert torch.equal(tap, t_tap) and (not win or torch.equal(pooled, t_pooled))
    assert float(tap[:, 0].abs().max()) == 0.0 and (not win or float(pooled[:, 0].abs().max()) == 0.0) and float(tap.max()) > 0
    rs = np.random.RandomState(5)
    ph, pw = _pool_shape(h, w, win)
    d_tap, d_pooled = rs.randn(n, c, h, w).astype(np.float32), rs.randn(n, c, ph, pw).astype(np.float32)
    combos = [("d_tap", d_tap, None)] + ([("d_pooled", None, d_pooled), ("both", d_tap, d_pooled)] if win else [])
    for name, dt, dp in combos:
        dtd, dpd = (None if dt is None else _dev(dt)), (None if dp is None else _dev(dp))
        got = _launch_pool_bwd(tap, dtd, dpd, win)
        assert got.tobytes() == _launch_pool_bwd(tap, dtd, dpd, win).tobytes()
        t = lambda a: None if a is None else torch.from_numpy(a)
        want = lr.pool_ref(torch.from_numpy(x), torch.from_numpy(b), win, torch.float64, t(dt), t(dp))[2].numpy()
        t32 = lr.pool_ref(xd, bd, win, torch.float32, dtd, dpd)[2].cpu().numpy()
        _within(got, want, cr.bound(t32, want), f"relu_pool backward {name}")
        assert float(np.abs(got[:, 0]).max()) == 0.0 and np.all(got[tap.cpu().numpy() == 0] == 0.0) and np.any(got != 0)
        if n == 2:                                                         # sample 1 alone: the same bytes
            one = _launch_pool_bwd(tap[1:].contiguous(), None if dtd is None else dtd[1:].contiguous(), None if dpd is None else dpd[1:].contiguous(), win)
            assert one.tobytes() == got[1:].tobytes()
    if n == 2:
        one_tap, one_pooled = _launch_pool(xd[1:].contiguous(), bd, win)
        assert torch.equal(one_tap, tap[1:]) and torch.equal(one_pooled, pooled[1:])


@pytest.mark.parametrize("h,win", [(8, 2), (9, 3)])
def test_relu_pool_ties_go_to_the_first_maximum_as_in_torch(h, win):
    """Small integers: positive ties in most windows, integer gradients -- every sum is exact, so the backward equals torch's."""
    rs = np.random.RandomState(3)
    x = rs.randint(-2, 3, [2, 4, h, h]).astype(np.float32)
    b = rs.randint(-1, 2, [4]).astype(np.float32)
    xd, bd = _dev(x), _dev(b)
    tap, pooled = _launch_pool(xd, bd, win)
    ph, pw = _pool_shape(h, h, win)
    d_tap, d_pooled = _dev(rs.randint(-3, 4, [2, 4, h, h]).astype(np.float32)), _dev(rs.randint(-3, 4, [2, 4, ph, pw]).astype(np.float32))
    patches = F.unfold(tap.reshape(-1, 1, h, h), win, stride=2)
    top = patches.topk(2, dim=1).values
    assert int(((top[:, 0] == top[:, 1]) & (top[:, 0] > 0)).sum()) >= 16          # the case has positive ties
    for dt, dp in ((d_tap, d_pooled), (None, d_pooled)):
        got = _launch_pool_bwd(tap, dt, dp, win)
        want = lr.pool_ref(xd, bd, win, torch.float32, dt, dp)[2].cpu().numpy()
        assert got.tobytes() == want.tobytes()


# ------------------------------------------------------------------------------------------------
# head
# ------------------------------------------------------------------------------------------------
def _launch_head(f0, f1, w, g, accumulate_into=None):
    n, c, h, wd = f0.shape
    hw = h * wd
    parts = int(_lib.lib().nb_lpips_head_parts(c, hw))
    kept, partials, acc, d_f1 = Guarded(3 * n * hw), Guarded(n * parts), Guarded(n), Guarded(f1.numel())
    acc.view.zero_()
    lib = _lib.lib()
    first = None
    for _level in range(2):                                                # two levels' worth: the finish ADDS
        _lib.check(lib.nb_lpips_head_f32(f0.data_ptr(), f1.data_ptr(), w.data_ptr(), n, c, hw, kept.view.data_ptr(), partials.view.data_ptr(),
                                         acc.view.data_ptr(), _st()), "lpips_head")
        first = acc.view.clone() if first is None else first
    if accumulate_into is not None:
        d_f1.view.copy_(accumulate_into.reshape(-1))
    _lib.check(lib.nb_lpips_head_bwd_f32(f0.data_ptr(), f1.data_ptr(), w.data_ptr(), kept.view.data_ptr(), g.data_ptr(), n, c, hw,
                                         int(accumulate_into is not None), d_f1.view.data_ptr(), _st()), "lpips_head_bwd")
    torch.cuda.synchronize()
    assert all(x.intact() for x in (kept, partials, acc, d_f1))
    assert torch.equal(acc.view, first + first)
    return first.cpu().numpy(), d_f1.view.view(n, c, h, wd).cpu().numpy(), kept.view.view(3, n, hw).cpu().numpy()


@pytest.mark.parametrize("n,c,h,w", lr.HEAD_CASES, ids=[f"n{n}_c{c}_{h}x{w}" for n, c, h, w in lr.HEAD_CASES])
def test_head_entries(n, c, h, w):
    f0, f1, wv, g = lr.head_case(n, c, h, w)
    split = h * w <= _lib.NB_LPIPS_SPLIT_MAX_HW and c >= _lib.NB_LPIPS_SPLIT_MIN_C
    assert split == ((n, c, h, w) in [(2, 64, 15, 15), (2, 512, 2, 2)]) and np.any(wv < 0)
    parts = int(_lib.lib().nb_lpips_head_parts(c, h * w))
    assert parts == (-(-h * w // 16) if split else -(-h * w // 256))
    a, b, wd, gd = _dev(f0), _dev(f1), _dev(wv), _dev(g)
    got = _launch_head(a, b, wd, gd)
    again = _launch_head(a, b, wd, gd)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(got, again))
    # float64 statement (autograd and closed form), and the float32 torch route on the same device tensors
    b64 = torch.from_numpy(f1.astype(np.float64)).requires_grad_(True)
    want = lr.head_f64(f0, b64, wv)
    auto64, = torch.autograd.grad((want * torch.from_numpy(g.astype(np.float64))).sum(), b64)
    d64 = lr.head_bwd_f64(f0, f1, wv, g)
    assert np.abs(auto64.numpy() - d64).max() <= 1e-12 * np.abs(d64).max()
    b32 = b.clone().requires_grad_(True)
    out32 = perceptual.head_torch(a, b32, wd)
    d32, = torch.autograd.grad((out32 * gd).sum(), b32)
    _within(got[0], want.detach().numpy(), cr.bound(out32.detach().cpu().numpy(), want.detach().numpy()), "head value")
    _within(got[1], d64, cr.bound(d32.cpu().numpy(), d64), "head d_f1")
    if h * w >= 3:                                                         # zero pixels: f0 only, f1 only, both
        flat, k = got[1].reshape(n, c, -1), got[2]
        assert np.all(flat[0, :, 1] == 0) and np.all(flat[0, :, 2] == 0) and np.any(flat[0, :, 0] != 0)
        assert k[0, 0, 0] == 0 and k[0, 0, 2] == 0 and k[1, 0, 1] == 0 and k[1, 0, 2] == 0 and k[0, 0, 1] > 0 and k[1, 0, 0] > 0
    ones = torch.ones_like(b)
    acc = _launch_head(a, b, wd, gd, accumulate_into=ones)[1]
    assert acc.tobytes() == (ones + _dev(got[1])).cpu().numpy().tobytes()
    for i in range(n if n > 1 else 0):                                     # sample i alone: the same bytes
        one = _launch_head(a[i:i + 1].contiguous(), b[i:i + 1].contiguous(), wd, gd[i:i + 1].contiguous())
        assert one[0].tobytes() == got[0][i:i + 1].tobytes() and one[1].tobytes() == got[1][i:i + 1].tobytes()


# ------------------------------------------------------------------------------------------------
# whole network
# ------------------------------------------------------------------------------------------------
_NETWORK = {}


def _network_reference(arch):
    """Once per case (lpips_refs.SLIM): the case, the float64 statement with its kink margins and the sign pattern of its five taps
    (CPU), and the float32 torch route on the device."""
    if arch not in _NETWORK:
        w, x0, x1 = lr.network_case(arch)
        rec64, rec32 = [], []
        a64 = torch.from_numpy(x1.astype(np.float64)).requires_grad_(True)
        v64 = lr.lpips_f64(w, x0, a64, record=rec64)
        g64, = torch.autograd.grad(v64.sum(), a64)
        lr.lpips_f64(w, x0, torch.from_numpy(x1), dtype=torch.float32, record=rec32)
        net32 = perceptual.LPIPS(w, route="torch", device=DEV)
        a32 = _dev(x1).requires_grad_(True)
        v32 = net32(_dev(x0), a32)
        g32, = torch.autograd.grad(v32.sum(), a32)
        live64 = [pre > 0 for (pre, _win), lay in zip(rec64, lr.layout(lr.SLIM[arch].get("arch", arch))) if lay[4] is not None]
        _NETWORK[arch] = dict(w=w, x0=x0, x1=x1, margins=lr.kink_margins(rec64, rec32), v64=v64.detach().numpy(), g64=g64.numpy(), live64=live64,
                              v32=v32.detach().cpu().numpy(), g32=g32.cpu().numpy())
    return _NETWORK[arch]


@pytest.mark.parametrize("split_f16", [False, True], ids=["fp32", "split_f16"])
@pytest.mark.parametrize("arch", ["vgg", "alex", "vgg64"])
def test_network_routes_against_float64(arch, split_f16, monkeypatch):
    """"vgg" and "alex" are below ops.TRAIN_SPLIT_F16_MIN_PIXELS: no split-path branch runs with either setting.  "vgg64" runs its two
    64 x 64 layers on the split-f16 up = 1 kernel, with the device ``tf`` weight pack in the backward (lpips_refs.NETWORK_BRANCHES)."""
    ref = _network_reference(arch)
    min_pre, min_gap, err = ref["margins"]
    print(f"[lpips] {arch}: smallest |pre-activation| {min_pre:.3g}, smallest pool gap {min_gap:.3g}, float32 pre-activation error {err:.3g}")
    assert min_pre >= lr.KINK_MARGIN * err and min_gap >= lr.KINK_MARGIN * err          # no ReLU / pool decision within reach of rounding
    monkeypatch.setattr(ops, "TRAIN_SPLIT_F16", split_f16)
    rec = split_branches.record(monkeypatch)
    net = perceptual.LPIPS(ref["w"], device=DEV)
    assert net.route == "hip"
    x0, a = _dev(ref["x0"]), _dev(ref["x1"]).requires_grad_(True)
    got = net(x0, a)
    assert got.shape == (x0.shape[0],)
    g, = torch.autograd.grad(got.sum(), a)
    torch.cuda.synchronize()
    print(f"[lpips] {arch} split_f16={split_f16}: branches {sorted(rec)}")
    split_branches.check(split_f16, rec, lr.NETWORK_BRANCHES[arch], f"{arch} network")
    # no ReLU decision flipped: the taps of the second image are positive exactly where the float64 statement's are
    taps = net.target_taps(_dev(ref["x1"]))
    assert len(taps) == 5 and all(torch.equal((t > 0).cpu(), l64) for t, l64 in zip(taps, ref["live64"])), f"{arch}: a ReLU decision differs from float64"
    factor = lr.SPLIT_F16_FACTOR / cr.BOUND_FACTOR if split_f16 else 1.0
    for name, mine, t32, f64 in (("value", got.detach().cpu().numpy(), ref["v32"], ref["v64"]), ("gradient", g.cpu().numpy(), ref["g32"], ref["g64"])):
        e32, e = float(np.abs(t32.astype(np.float64) - f64).max()), float(np.abs(mine.astype(np.float64) - f64).max())
        print(f"[lpips] {arch} split_f16={split_f16} {name}: kernel error {e:.3g}, float32 torch route error {e32:.3g}, ratio {e / max(e32, 1e-300):.3g}")
        _within(mine, f64, factor * cr.BOUND_FACTOR * e32 + cr.ULP_FLOOR * cr.EPS32 * np.abs(f64), f"{arch} network {name}")
    # bind against unbound: the same launches on the same taps
    bound = net.bind(x0)
    calls = net.trunk_calls
    b = _dev(ref["x1"]).requires_grad_(True)
    again = bound(x0, b)
    gb, = torch.autograd.grad(again.sum(), b)
    assert net.trunk_calls == calls + 1 and torch.equal(again, got) and torch.equal(gb, g)
    # per-sample upstream gradients reach the right samples
    up = torch.arange(1, x0.shape[0] + 1, dtype=torch.float32, device=DEV)
    c = _dev(ref["x1"]).requires_grad_(True)
    gs, = torch.autograd.grad((bound(x0, c) * up).sum(), c)
    assert float((gs - g * up.reshape(-1, 1, 1, 1)).abs().max()) <= 1e-5 * float(gs.abs().max())


# ------------------------------------------------------------------------------------------------
# wiring
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny():
    from brushstroke_engine_amd.training import TrainableGenerator
    cfg = cfgmod.tiny_config(32)
    sd = wmod.random_state_dict(cfg, 5)
    w = lr.network_case("vgg")[0]
    nets = {route: perceptual.LPIPS(w, route=route, device=DEV) for route in ("hip", "torch")}
    return cfg, TrainableGenerator(cfg, sd, DEV).requires_grad_(False), cr.StandInEncoder(cfg), nets


def _arenas_agree(res, what):
    scale = float(np.abs(res["torch"][0]).max())
    err = float(np.abs(res["hip"][0] - res["torch"][0]).max())
    print(f"[lpips] {what}: gradient arenas differ by {err:.3g}, largest gradient {scale:.3g}")
    assert scale > 0 and err <= 1e-5 * scale
    assert np.allclose(res["hip"][1], res["torch"][1], rtol=1e-4, atol=1e-7)


def test_projector_gradient_hip_route_against_torch_route(tiny):
    cfg, T, enc, nets = tiny
    k, b = 2, 3
    exs = [pr.exemplar(32, b, seed=31), pr.exemplar(32, b, seed=32)]
    kw = dict(w_plus=True, with_composite=True, w_avg=np.zeros([1, 1, cfg.w_dim]), w_std=1.0)
    lo = projection.BrushProjector(T, enc, route="torch", perceptual=nets["torch"], **kw).layout
    rs = np.random.RandomState(6)
    arena, w_noise = rs.randn(k, lo.p).astype(np.float32), 0.05 * rs.randn(k, *lo.w_shape).astype(np.float32)
    res = {}
    for route in ("hip", "torch"):
        p = projection.BrushProjector(T, enc, route=route, perceptual=nets[route], **kw)
        out = p.loss_and_grad(_dev(arena), _dev(w_noise), p.prepare(exs))
        res[route] = [x.cpu().numpy() for x in out]
    assert np.all(res["torch"][1][:, 2] > 0)
    _arenas_agree(res, "projector")


def test_clarity_gradient_hip_route_against_torch_route(tiny):
    cfg, T, enc, nets = tiny
    k, b = 2, 3
    drawings = cr.line_drawings(32, b, seed=2)
    lo = clarity.ArenaLayout.from_config(cfg)
    rs = np.random.RandomState(6)
    arena = rs.randn(k, lo.p).astype(np.float32)
    w_start = arena[:, :lo.nw].reshape(k, *lo.w_shape) + 0.1 * rs.randn(k, *lo.w_shape).astype(np.float32)
    w_noise = 0.05 * rs.randn(k, *lo.w_shape).astype(np.float32)
    geom = _dev(drawings.astype(np.float32) / 255)[:, None]
    res = {}
    for route in ("hip", "torch"):
        opt = clarity.ClarityOptimizer(T, enc, drawings, losses=clarity.DEFAULT_LOSSES + "+50*lpips(fake_orig)", route=route, w_std=1.0, lpips=nets[route])
        assert opt.fused and opt.item_names[3] == "lpips_fake_orig"
        out = opt.loss_and_grad(_dev(arena), _dev(w_start), _dev(w_noise), geom)
        res[route] = [x.cpu().numpy() for x in out]
    assert np.all(res["torch"][1][:, 3] > 0)
    _arenas_agree(res, "clarity")


def test_three_step_projection_lowers_the_perceptual_value(tiny):
    """Step 0 has learning rate 0 (the ramp-up), so the third evaluation is the first after a real update; no W noise, a small rate."""
    cfg, T, enc, nets = tiny
    p = projection.BrushProjector(T, enc, perceptual=nets["hip"], num_steps=3, w_plus=True, with_composite=True, w_avg=np.zeros([1, 1, cfg.w_dim]),
                                  w_std=1.0, initial_learning_rate=0.02, initial_noise_factor=0.0)
    assert p.route == "hip"
    seen = []
    calls = nets["hip"].trunk_calls
    out = p.project({"a": pr.exemplar(32, 3, seed=31), "b": pr.exemplar(32, 3, seed=32)}, brushes_per_pass=2, seed=1,
                    on_step=lambda ids, s, lr_, items, reg: seen.append(items[:, 2].cpu().numpy()))
    assert nets["hip"].trunk_calls == calls + 1 + 3 and len(seen) == 3 and sorted(out) == ["a", "b"]
    print(f"[lpips] perceptual per step: {[s.tolist() for s in seen]}")
    assert np.all(np.isfinite(seen)) and np.all(seen[2] < seen[0])
