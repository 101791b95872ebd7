"""GPU: the clarity kernels (csrc/nb_clarity.hip) against the float64 statement of tests/clarity_refs.py at the smallest shapes that
can go wrong, ``TrainableGenerator.synthesis(noise_buffers=...)`` against float64 autograd through the oracle, and
``clarity.ClarityOptimizer`` on the HIP generator: route "hip" against route "torch" from the same state, and a short run whose
result paints.

Bound of every kernel quantity (clarity_refs.bound): BOUND_FACTOR x the error of the float32 torch route on the same inputs against
float64 -- the kernels sum in another order -- plus ULP_FLOOR float32 ulps of the value.  Outputs sit between sentinel guards, inputs
are strided or offset views where the entry takes a stride, two launches give the same bytes, and row k of a K = 2 launch is the
K = 1 launch on that row."""
import ctypes as C

import numpy as np
import pytest
import torch

import clarity_refs as cr
from brushstroke_engine_amd import _lib, clarity, config as cfgmod, encoder as encmod, formats, painting, weights as wmod

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


def _within(got, want, bnd, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err = np.abs(got - want)
    worst = int(np.argmax(err - bnd))
    print(f"[clarity] {what}: max err {err.max():.3g}, smallest bound {np.min(bnd):.3g}, worst err/bound {(err / np.maximum(bnd, 1e-300)).max():.3g}")
    assert np.all(np.isfinite(got)) and np.all(err <= bnd), (what, err.reshape(-1)[worst], np.broadcast_to(bnd, err.shape).reshape(-1)[worst])


# ------------------------------------------------------------------------------------------------
# loss
# ------------------------------------------------------------------------------------------------
def _loss_views(c):
    """The case's tensors on the device: uvs as channels 1..3 of a NaN-filled [n,5,r,r] tensor, img one float behind a 16-byte boundary,
    target dense."""
    n, r = c["k"] * c["b"], c["r"]
    big = torch.full([n, 5, r, r], float("nan"), dtype=torch.float32, device=DEV)
    big[:, 1:4] = torch.from_numpy(c["uvs"]).to(DEV)
    flat = torch.full([n * 3 * r * r + 8], float("nan"), dtype=torch.float32, device=DEV)
    img = flat[1:1 + n * 3 * r * r].view(n, 3, r, r)
    img.copy_(torch.from_numpy(c["img"]))
    return big[:, 1:4], img, torch.from_numpy(c["target"]).to(DEV), torch.from_numpy(c["geom"]).to(DEV)


def _launch_loss(uvs, img, target, geom, k, b, r, w, gscale=None):
    n = k * b
    out, sums, parts = Guarded(4 * k), Guarded(8 * n), Guarded(n * _lib.NB_CLARITY_LOSS_PARTS * 8)
    d_uvs, d_img = Guarded(n * 3 * r * r), Guarded(n * 3 * r * r)
    lib = _lib.lib()
    _lib.check(lib.nb_clarity_loss_f32(uvs.data_ptr(), uvs.stride(0), img.data_ptr(), img.stride(0), target.data_ptr(), target.stride(0),
                                       geom.data_ptr(), k, b, r, w[0], w[1], w[2], out.view.data_ptr(), sums.view.data_ptr(), parts.view.data_ptr(),
                                       _st()), "clarity_loss")
    _lib.check(lib.nb_clarity_loss_bwd_f32(img.data_ptr(), img.stride(0), target.data_ptr(), target.stride(0), geom.data_ptr(), sums.view.data_ptr(),
                                           None if gscale is None else gscale.data_ptr(), k, b, r, w[0], w[1], w[2], d_uvs.view.data_ptr(),
                                           d_img.view.data_ptr(), _st()), "clarity_loss_bwd")
    torch.cuda.synchronize()
    assert all(g.intact() for g in (out, sums, parts, d_uvs, d_img))
    return (out.view.view(k, 4).cpu().numpy(), d_uvs.view.view(n, 3, r, r).cpu().numpy(), d_img.view.view(n, 3, r, r).cpu().numpy())


@pytest.mark.parametrize("r,b,k", cr.LOSS_CASES, ids=[f"r{r}_b{b}_k{k}" for r, b, k in cr.LOSS_CASES])
def test_loss_entries(r, b, k):
    c = cr.loss_case(r, b, k)
    w = c["weights"]
    uvs, img, target, geom = _loss_views(c)
    gscale = torch.tensor([1.0, 0.25][:k], dtype=torch.float32, device=DEV)
    got = _launch_loss(uvs, img, target, geom, k, b, r, w, gscale)
    again = _launch_loss(uvs, img, target, geom, k, b, r, w, gscale)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(got, again))
    # float64 statement, and the float32 torch route on the same device tensors
    out64, sums64 = cr.loss_f64(c["uvs"], c["img"], c["target"], c["geom"], k, w)
    du64, di64 = cr.loss_bwd_f64(c["img"], c["target"], c["geom"], sums64, k, w, gscale.cpu().numpy())
    u32, i32 = uvs.clone().requires_grad_(True), img.clone().requires_grad_(True)
    out32 = clarity.loss_torch(u32, i32, target, geom, k, w)
    (out32[:, 3] * gscale).sum().backward()
    _within(got[0], out64.numpy(), cr.bound(out32.detach().cpu().numpy(), out64.numpy()), "loss out")
    _within(got[1], du64, cr.bound(u32.grad.cpu().numpy(), du64), "d_uvs")
    _within(got[2], di64, cr.bound(i32.grad.cpu().numpy(), di64), "d_img")
    assert np.all(got[1][:, 1] == 0.0)
    # sign(0) = 0 where the target equals the image
    assert np.all(got[2][:, :, : r // 2, : r // 3] == 0.0) and np.any(got[2] != 0.0)
    if k == 2:                                                            # row 1 alone: the same bytes
        n1 = slice(b, 2 * b)
        one = _launch_loss(uvs[n1], img[n1], target[n1], geom, 1, b, r, w, gscale[1:])
        assert one[0].tobytes() == got[0][1:].tobytes() and one[1].tobytes() == got[1][n1].tobytes() and one[2].tobytes() == got[2][n1].tobytes()


def test_fused_loss_function_matches_torch_route():
    """The autograd.Function around the two entries: values and gradients as ``loss_torch`` gives them, on non-contiguous inputs."""
    c = cr.loss_case(20, 3, 2)
    uvs, img, target, geom = _loss_views(c)
    a, b_ = uvs.clone().requires_grad_(True), img.clone().requires_grad_(True)
    total, items = clarity.fused_clarity_loss(a.transpose(2, 3).transpose(2, 3), b_, target, geom, 2, c["weights"])
    assert not items.requires_grad
    (total * torch.tensor([1.0, 0.25], device=DEV)).sum().backward()
    u32, i32 = uvs.clone().requires_grad_(True), img.clone().requires_grad_(True)
    out32 = clarity.loss_torch(u32, i32, target, geom, 2, c["weights"])
    (out32[:, 3] * torch.tensor([1.0, 0.25], device=DEV)).sum().backward()
    assert torch.allclose(total, out32[:, 3].detach(), rtol=1e-5, atol=0) and torch.allclose(items, out32[:, :3].detach(), rtol=1e-5, atol=1e-9)
    assert float((a.grad - u32.grad).abs().max()) <= 1e-5 * float(u32.grad.abs().max())
    assert float((b_.grad - i32.grad).abs().max()) <= 1e-5 * float(i32.grad.abs().max())


# ------------------------------------------------------------------------------------------------
# regulariser and step: rows inside wider buffers
# ------------------------------------------------------------------------------------------------
PAD = 3


def _rows(a, fill=float("nan")):
    """[K,P] host array as a view with row stride P + 8, starting PAD floats into each row of a filled buffer."""
    k, p = a.shape
    big = torch.full([k, p + 8], fill, dtype=torch.float32, device=DEV)
    big[:, PAD:PAD + p] = torch.from_numpy(np.asarray(a, np.float32)).to(DEV)
    return big, big[:, PAD:PAD + p]


def _margins_intact(big, p, fill):
    m = torch.cat([big[:, :PAD].reshape(-1), big[:, PAD + p:].reshape(-1)])
    return bool(torch.isnan(m).all()) if np.isnan(fill) else bool((m == fill).all())


def _scratch(lo, k):
    planes = lo.planes_struct()
    n = _lib.lib().nb_clarity_scratch_floats(C.byref(planes), lo.nw, lo.p, k)
    assert n > 0
    return planes, Guarded(int(n))


def _launch_reg(lo, arena_view, grad_view, k, weight):
    planes, scratch = _scratch(lo, k)
    reg = Guarded(k)
    _lib.check(_lib.lib().nb_noise_reg_f32(arena_view.data_ptr(), arena_view.stride(0), lo.p, lo.nw, C.byref(planes), k, weight,
                                           None if grad_view is None else grad_view.data_ptr(), 0 if grad_view is None else grad_view.stride(0),
                                           reg.view.data_ptr(), scratch.view.data_ptr(), scratch.view.numel(), _st()), "noise_reg")
    torch.cuda.synchronize()
    assert reg.intact() and scratch.intact()
    return reg.view.cpu().numpy()


def test_noise_reg_entry():
    lo, k, weight = cr.reg_layout(), 2, 10.0
    a = cr.reg_arena(k)
    base = np.random.RandomState(8).randn(k, lo.p).astype(np.float32) * 0.01
    abig, av = _rows(a)
    runs = []
    for _ in range(2):
        gbig, gv = _rows(base, fill=5.0)
        reg = _launch_reg(lo, av, gv, k, weight)
        assert _margins_intact(gbig, lo.p, 5.0) and _margins_intact(abig, lo.p, float("nan"))
        runs.append((reg, gv.cpu().numpy()))
    assert runs[0][0].tobytes() == runs[1][0].tobytes() and runs[0][1].tobytes() == runs[1][1].tobytes()
    reg, grad = runs[0]
    assert np.array_equal(grad[:, :lo.nw], base[:, :lo.nw])                # W+ takes no part
    # float64 statement; the float32 torch route on the device
    reg64 = cr.noise_reg_f64(a, lo).numpy()
    g64 = base.astype(np.float64) + weight * cr.noise_reg_grad_f64(a, lo)
    a32 = torch.from_numpy(a).to(DEV).requires_grad_(True)
    reg32 = clarity.noise_reg_torch(a32, lo)
    reg32.sum().backward()
    g32 = (torch.from_numpy(base).to(DEV) + weight * a32.grad).cpu().numpy()
    _within(reg, reg64, cr.bound(reg32.detach().cpu().numpy(), reg64), "reg value")
    _within(grad, g64, cr.bound(g32, g64), "reg gradient")
    # the plane that is non-zero only on its border: its level-0 sums come from wrapped products alone, and are not zero
    edge = a[0, lo.off[5]:lo.off[5] + 1024].reshape(32, 32).astype(np.float64)
    assert abs((edge * np.roll(edge, 1, 1)).mean()) > 0 and abs((edge[1:-1] * np.roll(edge, 1, 1)[1:-1])[:, 1:].sum()) == 0
    # value only (no gradient arena), and row 1 alone
    assert _launch_reg(lo, av, None, k, weight).tobytes() == reg.tobytes()
    gbig1, gv1 = _rows(base[1:], fill=5.0)
    reg1 = _launch_reg(lo, av[1:], gv1, 1, weight)
    assert reg1.tobytes() == reg[1:].tobytes() and gv1.cpu().numpy().tobytes() == grad[1:].tobytes()


@pytest.mark.parametrize("t", [1, 2, 10])
def test_step_entry(t):
    lo, k, lr = cr.reg_layout(), 2, 0.07
    rs = np.random.RandomState(20 + t)
    a = cr.reg_arena(k, seed=4)
    g = (rs.randn(k, lo.p) * 1e-3).astype(np.float32)
    g[:, lo.off[3]:lo.off[3] + lo.res[3] ** 2] = 0.0                       # a plane without gradient
    m = np.zeros_like(g) if t == 1 else (rs.randn(k, lo.p) * 1e-3).astype(np.float32)
    v = np.zeros_like(g) if t == 1 else ((np.abs(rs.randn(k, lo.p)) + 0.5) * 1e-6).astype(np.float32)
    if t > 1:
        m[:, lo.off[3]:lo.off[3] + lo.res[3] ** 2] = 0.0
        v[:, lo.off[3]:lo.off[3] + lo.res[3] ** 2] = 0.0

    def launch(rows):
        k_ = rows.stop - rows.start
        bufs = [_rows(x[rows]) for x in (a, g, m, v)]
        planes, scratch = _scratch(lo, k_)
        views = [b[1] for b in bufs]
        assert len({x.stride(0) for x in views}) == 1
        _lib.check(_lib.lib().nb_clarity_step_f32(views[0].data_ptr(), views[1].data_ptr(), views[2].data_ptr(), views[3].data_ptr(), views[0].stride(0),
                                                  lo.p, lo.nw, C.byref(planes), k_, lr, t, scratch.view.data_ptr(), scratch.view.numel(), _st()), "clarity_step")
        torch.cuda.synchronize()
        assert scratch.intact() and all(_margins_intact(b[0], lo.p, float("nan")) for b in bufs)
        assert views[1].cpu().numpy().tobytes() == g[rows].tobytes()      # the gradient is read only
        return [views[i].cpu().numpy() for i in (0, 2, 3)]

    got, again = launch(slice(0, k)), launch(slice(0, k))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(got, again))
    one = launch(slice(1, 2))
    assert all(x.tobytes() == y[1:].tobytes() for x, y in zip(one, got))
    want = cr.step_f64(a, g, m, v, lo, lr, t)
    t32 = [torch.from_numpy(x.copy()).to(DEV) for x in (a, g, m, v)]
    clarity.step_torch(t32[0], t32[1], t32[2], t32[3], lo, lr, t)
    for name, x, w64, x32 in zip(("arena", "m", "v"), got, want, (t32[0], t32[2], t32[3])):
        _within(x, w64, cr.bound(x32.cpu().numpy(), w64), f"step t={t} {name}")
    for i, (r, o) in enumerate(zip(lo.res, lo.off)):                       # every plane: zero mean, unit mean square
        n = got[0][:, o:o + r * r].astype(np.float64)
        assert np.all(np.abs(n.mean(axis=1)) <= 8 * cr.EPS32) and np.all(np.abs((n * n).mean(axis=1) - 1) <= cr.mean_square_tol(r)), i


# ------------------------------------------------------------------------------------------------
# the differentiable generator with noise buffers
# ------------------------------------------------------------------------------------------------
def test_trainable_synthesis_noise_buffers_against_float64_oracle():
    """Image and gradients with respect to ws, a per-sample plane and a shared plane, against float64 autograd through the oracle; the
    tolerance of the whole-generator gradient test (tests/test_hip_training.py: 2e-5 on the image, 2e-4 of each gradient's scale)."""
    from brushstroke_engine_amd.training import TrainableGenerator
    from brushstroke_engine_amd import synthetic
    from oracle import neube_oracle as orc
    cfg, n = cfgmod.tiny_config(32), 2
    sd = wmod.random_state_dict(cfg, 5)
    rs = np.random.RandomState(2)
    ws = rs.randn(n, cfg.num_ws, cfg.w_dim)
    geom = [g.astype(np.float64) for g in synthetic.geom_features(cfg, n, 7)]
    per_sample, shared = rs.randn(n, 1, 16, 16), rs.randn(32, 32)
    weight = rs.randn(n, 3, 32, 32)

    def run(gen_synthesis, dtype, dev):
        t = lambda x: torch.tensor(x, dtype=dtype, device=dev)
        w, a, b = t(ws).requires_grad_(True), t(per_sample).requires_grad_(True), t(shared).requires_grad_(True)
        img, dbg = gen_synthesis(w, [t(g) for g in geom], {"b16.conv0.noise_const": a, "b32.conv1.noise_const": b})
        grads = torch.autograd.grad((img * t(weight)).sum() + dbg["uvs"][:, 2].square().sum(), [w, a, b])
        return img.detach().cpu().double(), [x.cpu().double() for x in grads]

    O = orc.OracleGenerator(cfg, sd, torch.float64)
    want_img, want = run(lambda w, g, nb: O.synthesis(w, g, return_debug_data=True, noise_buffers=nb), torch.float64, "cpu")
    T = TrainableGenerator(cfg, sd, DEV)
    got_img, got = run(lambda w, g, nb: T.synthesis(w, g, noise_mode="const", noise_buffers=nb, return_debug_data=True), torch.float32, DEV)
    assert float((got_img - want_img).abs().max()) <= 2e-5 * max(1.0, float(want_img.abs().max()))
    for name, a, b in zip(("ws", "per-sample noise", "shared noise"), got, want):
        scale, err = float(b.abs().max()), float((a - b).abs().max())
        print(f"[clarity] noise_buffers gradient {name}: err {err:.3g}, scale {scale:.3g}")
        assert a.shape == b.shape and err <= 2e-4 * scale + 1e-9, (name, err, scale)
    with torch.no_grad():                                                  # None changes nothing; an unknown key or a wrong shape raises
        w32 = torch.tensor(ws, dtype=torch.float32, device=DEV)
        g32 = [torch.tensor(g, dtype=torch.float32, device=DEV) for g in geom]
        assert torch.equal(T.synthesis(w32, g32, noise_mode="const"), T.synthesis(w32, g32, noise_mode="const", noise_buffers=None))
        with pytest.raises(KeyError):
            T.synthesis(w32, g32, noise_mode="const", noise_buffers={"b64.conv0.noise_const": torch.zeros(64, 64, device=DEV)})
        with pytest.raises(ValueError):
            T.synthesis(w32, g32, noise_mode="const", noise_buffers={"b16.conv0.noise_const": torch.zeros(8, 8, device=DEV)})


# ------------------------------------------------------------------------------------------------
# the optimiser on the HIP generator
# ------------------------------------------------------------------------------------------------
def test_gradient_arena_hip_route_against_torch_route():
    """From identical state and draws: the generator is the same, only loss and regulariser differ.  Bound as above, the float32
    torch route's error being measured against the float64 statement on the oracle (CPU)."""
    from brushstroke_engine_amd.training import TrainableGenerator
    cfg, k, b = cfgmod.tiny_config(32), 2, 3
    sd = wmod.random_state_dict(cfg, 5)
    T = TrainableGenerator(cfg, sd, DEV).requires_grad_(False)
    enc, drawings = cr.StandInEncoder(cfg), cr.line_drawings(32, b, seed=2)
    lo = clarity.ArenaLayout.from_config(cfg)
    rs = np.random.RandomState(6)
    arena = rs.randn(k, lo.p).astype(np.float32)
    w_start = arena[:, :lo.nw].reshape(k, *lo.w_shape) + 0.1 * rs.randn(k, *lo.w_shape).astype(np.float32)
    w_noise = 0.05 * rs.randn(k, *lo.w_shape).astype(np.float32)
    geom = torch.from_numpy(drawings.astype(np.float32) / 255)[:, None]
    res = {}
    for route in ("hip", "torch"):
        opt = clarity.ClarityOptimizer(T, enc, drawings, route=route, w_std=1.0)
        grad, items, reg = opt.loss_and_grad(torch.from_numpy(arena).to(DEV), torch.from_numpy(w_start).to(DEV), torch.from_numpy(w_noise).to(DEV),
                                             geom.to(DEV))
        res[route] = (grad.cpu().numpy(), items.cpu().numpy(), reg.cpu().numpy())
    opt64 = clarity.ClarityOptimizer(cr.OracleGen(cfg, sd, torch.float64), enc, drawings, route="torch", w_std=1.0)
    g64, i64, r64 = (x.numpy() for x in opt64.loss_and_grad(torch.from_numpy(arena.astype(np.float64)), torch.from_numpy(w_start.astype(np.float64)),
                                                             torch.from_numpy(w_noise.astype(np.float64)), geom.double()))
    for name, j, w64 in (("gradient arena", 0, g64), ("items", 1, i64), ("reg", 2, r64)):
        _within(res["hip"][j], w64, cr.bound(res["torch"][j], w64), f"optimiser {name}")
    assert np.abs(g64[:, lo.nw:]).max() > 0 and np.abs(g64[:, :lo.nw]).max() > 0


def test_three_step_run_paints():
    """Route "hip" at the shipped shapes (style1_config(128), the HIP encoder): finite, every plane normalised, the library format, and
    the result paints through PaintingHelper with its noise set -- the same bytes as a checkpoint that holds those planes."""
    from brushstroke_engine_amd.networks import Generator
    from brushstroke_engine_amd.training import TrainableGenerator
    cfg = cfgmod.style1_config(128)
    sd, esd = wmod.random_state_dict(cfg, seed=0), encmod.random_encoder_state_dict(5)
    enc = encmod.HipGeometryEncoder(esd)
    drawings = cr.line_drawings(128, 4, seed=1, width=4)
    T = TrainableGenerator(cfg, sd, DEV)
    opt = clarity.ClarityOptimizer(T, enc.encode, drawings, w_avg_samples=64)
    assert opt.route == "hip" and opt.fused
    seen = []
    out = opt.optimize(formats.SeedBrushLibrary([3, 11], cfg.z_dim), num_steps=3, batch_size=2, brushes_per_pass=2, seed=1,
                       on_step=lambda ids, step, lr, items, reg: seen.append((step, items.cpu().numpy(), reg.cpu().numpy())))
    assert sorted(out) == ["11", "3"] and len(seen) == 3 and all(np.isfinite(s[1]).all() and np.isfinite(s[2]).all() for s in seen)
    assert all(p.requires_grad for p in T.parameters()) and all(p.grad is None for p in T.parameters())
    lo = opt.layout
    for sid, e in out.items():
        assert tuple(e["w"].shape) == (1, cfg.num_ws, cfg.w_dim) and sorted(e["noise"]) == sorted(lo.names) and bool(torch.isfinite(e["w"]).all())
        for name, r in zip(lo.names, lo.res):
            n = e["noise"][name].double()
            assert tuple(n.shape) == (r, r) and bool(torch.isfinite(n).all())
            assert abs(float(n.mean())) <= 8 * cr.EPS32 and abs(float((n * n).mean()) - 1) <= cr.mean_square_tol(r), (sid, name)
        assert set(opt.history[sid]) == {"first", "last"} and "noise_reg" in opt.history[sid]["last"]
    lib = formats.WBrushLibrary(out)
    geom = drawings[0][:, :, None]
    opts = painting.GanBrushOptions()
    lib.set_style("3", opts)
    assert sorted(opts.custom_args["noise_buffers"]) == sorted(lo.names)
    with torch.no_grad():
        ops = painting.TileOps(Generator(cfg, sd).to(DEV), enc)
        img = painting.PaintingHelper(ops, batch=2).paint_image(geom, opts, crop_margin=10)
        sd2 = dict(sd)
        sd2.update({"synthesis." + n: v.numpy() for n, v in out["3"]["noise"].items()})
        plain = painting.GanBrushOptions()
        plain.set_style_w(out["3"]["w"], "3")
        held = painting.PaintingHelper(painting.TileOps(Generator(cfg, sd2).to(DEV), enc), batch=2).paint_image(geom, plain, crop_margin=10)
    assert img.shape[:2] == (128, 128) and np.array_equal(img, held)
