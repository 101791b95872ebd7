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


@pytest.mark.parametrize("arch", ["vgg", "alex", "vgg64"])
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
    assert net.arch == lr.SLIM[arch].get("arch", arch) and net.route == "torch"
    a = torch.from_numpy(x1).requires_grad_(True)
    got = net(torch.from_numpy(x0), a)
    g, = torch.autograd.grad(got.sum(), a)
    assert got.shape == (x0.shape[0],) and got.dtype == torch.float32
    assert float((got.detach().double() - want).abs().max()) <= 1e-4 * float(want.max())
    assert float((g.double() - g64).abs().max()) <= 1e-3 * float(g64.abs().max())
    bound = net.bind(torch.from_numpy(x0))
    assert torch.equal(bound(torch.from_numpy(x0), a.detach()), got.detach())
    assert float(net(torch.from_numpy(x0), torch.from_numpy(x0)).abs().max()) == 0.0


def test_the_split_path_network_case_reaches_the_threshold_at_its_first_two_layers_only():
    """"vgg64": n h w of the two 64 x 64 layers is ops.TRAIN_SPLIT_F16_MIN_PIXELS itself; every later layer is below it."""
    from brushstroke_engine_amd import ops
    c = lr.SLIM["vgg64"]
    assert c["arch"] == "vgg" and c["channels"] == (4, 8, 12, 12, 16) and c["seed"] == 52 and sorted(lr.NETWORK_BRANCHES) == sorted(lr.SLIM)
    sizes, side = [], c["size"]
    for _i, _k, _s, _p, _lvl, win in lr.layout("vgg"):
        sizes.append(c["n"] * side * side)
        side = side // 2 if win else side
    assert sizes[:2] == [ops.TRAIN_SPLIT_F16_MIN_PIXELS] * 2 and max(sizes[2:]) < ops.TRAIN_SPLIT_F16_MIN_PIXELS
    # the older cases: below it at every 3 x 3 layer (alex's 11 x 11 stride-4 and 5 x 5 layers are on the generic kernel at any size)
    assert lr.SLIM["vgg"]["n"] * lr.SLIM["vgg"]["size"] ** 2 < ops.TRAIN_SPLIT_F16_MIN_PIXELS
    assert lr.SLIM["alex"]["n"] * lr.layer_out_size(lr.SLIM["alex"]["size"], 11, 4, 2) ** 2 < ops.TRAIN_SPLIT_F16_MIN_PIXELS


@pytest.mark.parametrize("case", lr.LAYER_CASES, ids=lr.LAYER_IDS)
def test_layer_case_operands_are_what_the_trunk_feeds_its_convolutions(case):
    """The stated properties of tests/test_hip_lpips_trunk_f64.py's operands, and that its bounds can catch an error."""
    name, n, ci, co, h, w_, k, s, p, fwd, bwd = case
    ref = lr.layer_reference(case)
    x, w, d = ref["x"], ref["w"], ref["d"]
    ho, wo = lr.layer_out_size(h, k, s, p), lr.layer_out_size(w_, k, s, p)
    assert tuple(x.shape) == (n, ci, h, w_) and tuple(w.shape) == (co, ci, k, k) and tuple(d.shape) == (n, co, ho, wo)
    assert all(t.dtype == torch.float32 and bool(torch.isfinite(t).all()) for t in (x, w, d))
    if ci == 3:                                                            # the scaled image: both signs, within (+-1 - shift) / scale
        lim = max((1 + abs(sh)) / sc for sh, sc in zip(lr.SHIFT, lr.SCALE))
        assert float(x.min()) < -1 and float(x.max()) > 1 and float(x.abs().max()) <= lim
    else:                                                                  # ReLU outputs: a third of zeros, per-sample scales 1, 2^-6
        assert float(x.min()) == 0.0 and 0.3 <= float((x == 0).float().mean()) <= 0.4
        assert all(float(x[i].max()) < 2.0 ** -6 * 8 for i in range(1, n, 2)) and all(float(x[i].max()) > 2 for i in range(0, n, 2))
    # the gradient: one survivor per 2 x 2 window, 1 / (h w), per-sample scales with an all-zero sample where n >= 4
    scales = [float(d[i].abs().max()) for i in range(n)]
    zero = [i for i in range(n) if scales[i] == 0.0]
    assert zero == ([i for i in range(n) if i % 4 == 3] if n >= 4 else [])
    live = d[[i for i in range(n) if i not in zero]]
    per_window = torch.nn.functional.avg_pool2d((live != 0).float(), 2, 2, ceil_mode=True, divisor_override=1)
    assert float(per_window.max()) <= 1.0
    frac = float((live == 0).float().mean())
    assert frac == 0.75 if (ho % 2 == 0 and wo % 2 == 0) else 0.70 <= frac <= 0.80, (name, frac)
    assert scales[0] <= 6.0 / (ho * wo) and scales[0] >= 1.0 / (ho * wo) and (n == 1 or scales[1] <= scales[0] * 2.0 ** -5)
    # the declared routes follow from the shapes (ops.conv2d's thresholds)
    from brushstroke_engine_amd import ops
    pow2 = ops._pow2(h) and ops._pow2(w_)
    big = n * ho * wo >= ops.TRAIN_SPLIT_F16_MIN_PIXELS
    want = set() if (k, s, p) != (3, 1, 1) or not big or min(ho, wo) < 16 else ({"split_up1"} if pow2 else {"split_canvas"})
    assert fwd == want and bwd == (want | {"tf_pack"} if want == {"split_up1"} else want)
    # zeroing one channel moves the float64 results by >= 20 bounds, in either mode's bound
    for split in (False, True):
        t_y, t_dx = lr.layer_bounds(case, ref, split)
        assert t_y.shape == ref["y"].shape and t_dx.shape == ref["dx"].shape
        assert float((ref["y"] - ref["y_bad"]).abs().max()) >= lr.CATCH_FACTOR * float(t_y.max())
        assert float((ref["dx"] - ref["dx_bad"]).abs().max()) >= lr.CATCH_FACTOR * float(t_dx.max())
    # the reference is float64 F.conv2d and its autograd: checked against a direct sum at one output and one input element
    x64, w64, d64 = x.double(), w.double(), d.double()
    xp = torch.nn.functional.pad(x64, (p, p, p, p))
    i, o, r, c_ = n - 1 - (1 if zero and (n - 1) in zero else 0), co - 1, ho - 1, wo // 2
    direct = float((xp[i, :, r * s:r * s + k, c_ * s:c_ * s + k] * w64[o]).sum())
    assert abs(direct - float(ref["y"][i, o, r, c_])) <= 1e-12 * float(ref["y_abs"][i, o, r, c_])
    a, rr, cc = ci - 1, h - 1, w_ - 1                                      # the last row and column: what the remainder padding yields
    tot = 0.0
    for u in range(ho):
        for v in range(wo):
            kr, kc = rr + p - u * s, cc + p - v * s
            if 0 <= kr < k and 0 <= kc < k:
                tot += float((d64[i, :, u, v] * w64[:, a, kr, kc]).sum())
    assert abs(tot - float(ref["dx"][i, a, rr, cc])) <= 1e-12 * max(float(ref["dx_abs"][i, a, rr, cc]), 1e-300)


def test_stride4_layer_cases_have_every_remainder():
    """alex's 11 x 11 stride-4 layer at image sides 63 .. 67: remainders 0, 1, 2, 3, 0 of perceptual._conv_input_grad's right / bottom
    padding (the slim whole-network case has 1 only)."""
    sides = sorted({c[4] for c in lr.LAYER_CASES if c[7] == 4})
    assert sides == [63, 64, 65, 66, 67] and {c[3] for c in lr.LAYER_CASES if c[7] == 4} == {8, 64}
    assert [lr.stride_remainder(sd, 11, 4, 2) for sd in sides] == [0, 1, 2, 3, 0] == [lr.STRIDE4_REMAINDERS[sd] for sd in sides]
    assert lr.stride_remainder(lr.SLIM["alex"]["size"], 11, 4, 2) == 1
    for sd in sides:                                                       # the remainder is what the zero-stuffed gradient lacks
        ho = lr.layer_out_size(sd, 11, 4, 2)
        stuffed = (ho - 1) * 4 + 1
        assert stuffed + lr.stride_remainder(sd, 11, 4, 2) + 2 * (11 - 1 - 2) - 11 + 1 == sd


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
