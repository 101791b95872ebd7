"""CPU: ``perceptual.LPIPS`` route "torch" against the float64 statement of tests/lpips_refs.py, the zero-norm convention, the weight
converter, and the wiring into ``forger_losses``, ``clarity.ClarityOptimizer`` and ``projection.BrushProjector``."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import clarity_refs as cr
import lpips_refs as lr
import projection_refs as pr
from brushstroke_engine_amd import clarity, config as cfgmod, forger_losses, perceptual, projection, weights as wmod

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def slim_vgg():
    return perceptual.LPIPS(lr.slim_weights("vgg", (4, 6, 8, 8, 8), 1), route="torch", device="cpu")


@pytest.mark.parametrize("arch", ["vgg", "alex"])
def test_torch_route_against_float64_statement(arch):
    """Values and the gradient of the second image.  The float32 route differs from the statement by rounding, 13 (5) layers deep:
    asserted at 1e-4 of the value and 1e-3 of the largest gradient on cases whose ReLU and pool decisions are the same in both
    precisions (lpips_refs.kink_margins, asserted here)."""
    w, x0, x1 = lr.network_case(arch)
    rec64, rec32 = [], []
    a64 = torch.from_numpy(x1.astype(np.float64)).requires_grad_(True)
    want = lr.lpips_f64(w, x0, a64, record=rec64)
    g64, = torch.autograd.grad(want.sum(), a64)
    lr.lpips_f64(w, x0, torch.from_numpy(x1), dtype=torch.float32, record=rec32)
    min_pre, min_gap, err = lr.kink_margins(rec64, rec32)
    print(f"[lpips] {arch}: smallest |pre-activation| {min_pre:.3g}, smallest pool gap {min_gap:.3g}, float32 pre-activation error {err:.3g}")
    assert min_pre >= lr.KINK_MARGIN * err and min_gap >= lr.KINK_MARGIN * err
    want = want.detach()
    assert float(want.min()) > 0 and float(g64.abs().max()) > 0
    net = perceptual.LPIPS(w, route="torch", device="cpu")
    assert net.arch == arch and net.route == "torch"
    a = torch.from_numpy(x1).requires_grad_(True)
    got = net(torch.from_numpy(x0), a)
    g, = torch.autograd.grad(got.sum(), a)
    assert got.shape == (x0.shape[0],) and got.dtype == torch.float32
    assert float((got.detach().double() - want).abs().max()) <= 1e-4 * float(want.max())
    assert float((g.double() - g64).abs().max()) <= 1e-3 * float(g64.abs().max())
    bound = net.bind(torch.from_numpy(x0))
    assert torch.equal(bound(torch.from_numpy(x0), a.detach()), got.detach())
    assert float(net(torch.from_numpy(x0), torch.from_numpy(x0)).abs().max()) == 0.0


def test_zero_norm_pixels_give_a_finite_zero_gradient():
    f0, f1, w, g = lr.head_case(3, 24, 2, 2)
    a = torch.from_numpy(f1).requires_grad_(True)
    out = perceptual.head_torch(torch.from_numpy(f0), a, torch.from_numpy(w))
    d, = torch.autograd.grad((out * torch.from_numpy(g)).sum(), a)
    want = lr.head_bwd_f64(f0, f1, w, g)
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(d).all())
    flat = d.reshape(3, 24, -1)
    assert bool((flat[0, :, 1] == 0).all()) and bool((flat[0, :, 2] == 0).all()) and bool((flat[0, :, 0] != 0).any())
    assert np.abs(d.numpy() - want).max() <= 1e-5 * np.abs(want).max()
    # ... and the statement's autograd agrees with its closed form
    a64 = torch.from_numpy(f1.astype(np.float64)).requires_grad_(True)
    d64, = torch.autograd.grad((lr.head_f64(f0, a64, w) * torch.from_numpy(g.astype(np.float64))).sum(), a64)
    assert np.abs(d64.numpy() - want).max() <= 1e-12 * np.abs(want).max()
    # an image whose first tap is zero everywhere (a large negative bias): the whole gradient is finite
    wts = lr.slim_weights("vgg", (4, 6, 8, 8, 8), 1)
    wts["features.2.bias"] = np.full_like(wts["features.2.bias"], -1e3)
    net = perceptual.LPIPS(wts, route="torch", device="cpu")
    x = torch.zeros(1, 3, 32, 32).requires_grad_(True)
    gx, = torch.autograd.grad(net(torch.ones(1, 3, 32, 32) * 0.5, x).sum(), x)
    assert bool(torch.isfinite(gx).all())


def test_converter_round_trips_synthetic_state_dicts(tmp_path):
    spec = importlib.util.spec_from_file_location("convert_lpips_weights", os.path.join(REPO, "tools", "convert_lpips_weights.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    for arch in ("vgg", "alex"):
        w = lr.slim_weights(arch, (4, 6, 8, 8, 8), 2)
        trunk = {k: torch.from_numpy(v) for k, v in w.items() if k.startswith("features.")}
        trunk["classifier.0.weight"] = torch.zeros(3, 3)                   # what the trunk's file also holds
        head = {f"lin{l}.model.1.weight": torch.from_numpy(w[f"lin{l}.weight"]).reshape(1, -1, 1, 1) for l in range(5)}
        torch.save(trunk, tmp_path / "trunk.pth")
        torch.save(head, tmp_path / "head.pth")
        out = tool.main(["--trunk", str(tmp_path / "trunk.pth"), "--head", str(tmp_path / "head.pth"), "--arch", arch, "--out", str(tmp_path / f"{arch}.npz")])
        with np.load(out) as z:
            assert str(z["arch"]) == arch and sorted(k for k in z.files if not k.startswith("scaling.")) == sorted(w)
            assert all(np.array_equal(z[k], w[k]) for k in w if k != "arch")
            assert np.allclose(z["scaling.shift"], lr.SHIFT) and np.allclose(z["scaling.scale"], lr.SCALE)
        x0, x1 = torch.rand(1, 3, 64, 64) * 2 - 1, torch.rand(1, 3, 64, 64) * 2 - 1
        assert torch.equal(perceptual.LPIPS(out, route="torch", device="cpu")(x0, x1), perceptual.LPIPS(w, route="torch", device="cpu")(x0, x1))
        del head["lin3.model.1.weight"]
        with pytest.raises(KeyError, match="lin3"):
            perceptual.convert_state_dicts(trunk, head, arch)
    with pytest.raises(ValueError, match="arch"):
        perceptual.LPIPS({k: v for k, v in w.items() if k != "arch"}, route="torch", device="cpu")
    with pytest.raises(Exception, match="needs a GPU"):
        perceptual.LPIPS(w, route="hip", device="cpu")


def test_forger_losses_with_a_network(slim_vgg):
    rs = np.random.RandomState(0)
    d = {k: torch.from_numpy(np.tanh(rs.randn(2, 3, 32, 32)).astype(np.float32)) for k in ("fake_img", "fake_orig", "fake", "fake_composite")}
    losses = forger_losses.ForgerLosses.create_from_string("2*lpips(fake_orig)+lpips(fake_composite)", lpips=slim_vgg)
    total, items = losses.compute(d, None)
    a, b = slim_vgg(d["fake_orig"], d["fake_img"]).mean(), slim_vgg(d["fake"], d["fake_composite"]).mean()
    assert torch.equal(items["lpips_fake_orig"], a) and torch.equal(items["lpips_fake_composite"], b) and torch.equal(total, 2 * a + b)
    assert losses.require_original_fake_image()
    w, item = forger_losses.parse_loss_item("0.5*lpips(patch)", lpips=slim_vgg)
    assert w == 0.5 and item.full_name() == "lpips_patch"
    with pytest.raises(RuntimeError, match="Unsupported component"):
        forger_losses.parse_loss_item("lpips(uvs)", lpips=slim_vgg)[1].compute(d, None)
    with pytest.raises(RuntimeError, match="needs the LPIPS network"):
        forger_losses.parse_loss_item("lpips(fake_orig)")
    with pytest.raises(RuntimeError, match="needs the LPIPS network"):
        forger_losses.ForgerLosses.create_from_string("plpips(fake_orig)", lpips=slim_vgg)


def test_clarity_optimizer_adds_the_perceptual_term_per_brush(slim_vgg):
    """``loss_and_grad`` with '...+50*lpips(fake_orig)' equals the hand-summed total: the three fused items of the run without the
    perceptual item, plus 50 x the per-brush mean of the network on (target, image), value and gradient."""
    cfg, k, b = cfgmod.tiny_config(32), 2, 2
    sd = wmod.random_state_dict(cfg, 5)
    gen, enc, drawings = cr.OracleGen(cfg, sd), cr.StandInEncoder(cfg), cr.line_drawings(32, b, seed=2)
    lo = clarity.ArenaLayout.from_config(cfg)
    rs = np.random.RandomState(6)
    arena = torch.from_numpy(rs.randn(k, lo.p).astype(np.float32))
    w_start = lo.w(arena).clone() + 0.1 * torch.from_numpy(rs.randn(k, *lo.w_shape).astype(np.float32))
    w_noise = 0.05 * torch.from_numpy(rs.randn(k, *lo.w_shape).astype(np.float32))
    geom = torch.from_numpy(drawings.astype(np.float32) / 255)[:, None]
    plain = clarity.ClarityOptimizer(gen, enc, drawings, route="torch", w_std=1.0)
    full = clarity.ClarityOptimizer(gen, enc, drawings, losses=clarity.DEFAULT_LOSSES + "+50*lpips(fake_orig)", route="torch", w_std=1.0, lpips=slim_vgg)
    assert full.fused and full.lpips_weight == 50.0 and full.item_names == list(plain.item_names) + ["lpips_fake_orig"]
    g0, i0, r0 = plain.loss_and_grad(arena, w_start, w_noise, geom)
    g1, i1, r1 = full.loss_and_grad(arena, w_start, w_noise, geom)
    # by hand
    a = arena.clone().requires_grad_(True)
    feats = [f.repeat(k, 1, 1, 1) for f in enc(geom)]
    with torch.no_grad():
        target, _ = gen.synthesis(full._ws(w_start, b), feats, noise_mode="const", noise_buffers=full.noise_buffers(arena, b), return_debug_data=True)
    img, _ = gen.synthesis(full._ws(lo.w(a) + w_noise, b), feats, noise_mode="const", noise_buffers=full.noise_buffers(a, b), return_debug_data=True)
    perc = slim_vgg(target, img).reshape(k, b).mean(dim=1)
    gp, = torch.autograd.grad(50.0 * perc.sum(), a)
    assert float(perc.detach().min()) > 0 and float(gp.abs().max()) > 0
    assert torch.equal(i1[:, :3], i0) and torch.equal(r1, r0) and torch.allclose(i1[:, 3], perc.detach(), rtol=1e-6, atol=0)
    assert float((g1 - (g0 + gp)).abs().max()) <= 1e-5 * float(g1.abs().max())
    # other strings with the item go item by item through ForgerLosses.compute; without a network the string raises as before
    other = clarity.ClarityOptimizer(gen, enc, drawings, losses="lpips(fake_orig)+0.5*iou(u)", route="torch", w_std=1.0, lpips=slim_vgg)
    assert not other.fused and other.item_names == ["lpips_fake_orig", "iou_u"]
    g2, i2, _ = other.loss_and_grad(arena, w_start, w_noise, geom)
    assert torch.allclose(i2[:, 0], perc.detach(), rtol=1e-5, atol=0) and bool(torch.isfinite(g2).all())
    with pytest.raises(RuntimeError, match="needs the LPIPS network"):
        clarity.ClarityOptimizer(gen, enc, drawings, losses=clarity.DEFAULT_LOSSES + "+50*lpips(fake_orig)", route="torch")


def test_projector_runs_the_target_through_the_trunk_once_per_pass(slim_vgg):
    cfg = cfgmod.tiny_config(32)
    sd = wmod.random_state_dict(cfg, 5)
    steps, exs = 3, {"a": pr.exemplar(32, 2, seed=31), "b": pr.exemplar(32, 2, seed=32), "c": pr.exemplar(32, 2, seed=33)}
    kw = dict(route="torch", w_avg=np.zeros([1, 1, cfg.w_dim]), w_std=1.0, num_steps=steps, with_composite=True)
    # both other weights may be zero when there is a perceptual item, as in the reference
    p = projection.BrushProjector(pr.OracleGen(cfg, sd), cr.StandInEncoder(cfg), perceptual=slim_vgg, **kw)
    before = slim_vgg.trunk_calls
    seen = []
    out = p.project(exs, brushes_per_pass=2, seed=1, on_step=lambda ids, s, lr_, items, reg: seen.append(items[:, 2].clone()))
    passes = 2
    assert slim_vgg.trunk_calls - before == passes * (1 + steps)           # the target once per pass, the image once per step
    assert sorted(out) == ["a", "b", "c"] and p.item_names == ["l1", "bg", "perceptual"] and all(bool((s > 0).all()) for s in seen)
    # a plain callable is called as before, with the target, every step
    calls = []
    plain = lambda target, synth: (calls.append(target.shape[0]), slim_vgg(target, synth))[1]
    before = slim_vgg.trunk_calls
    projection.BrushProjector(pr.OracleGen(cfg, sd), cr.StandInEncoder(cfg), perceptual=plain, **kw).project({"a": exs["a"]}, seed=1)
    assert calls == [2] * steps and slim_vgg.trunk_calls - before == 2 * steps
    # bound and unbound give the same values
    fix = p.prepare([exs["a"]])
    synth = torch.tanh(torch.randn(2, 3, 32, 32, generator=torch.Generator().manual_seed(0)))
    assert torch.equal(fix["perceptual"](fix["target"], synth), slim_vgg(fix["target"], synth))
    with pytest.raises(ValueError, match="bound to a target"):
        fix["perceptual"](fix["target"][:1], synth[:1])
