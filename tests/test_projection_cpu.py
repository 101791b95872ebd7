"""Brush projection without a GPU: the float64 statement against its own autograd and central differences, the torch route against
the statement and against the reference's ``project()`` (tests/golden/projection.npz), the projector's bookkeeping, the samplers, the
command line, and the host-side argument checks of the three C entries."""
import json
import os
import re

import numpy as np
import pytest
import torch

import clarity_refs as cr
import projection_refs as pr
from conftest import load_golden
from brushstroke_engine_amd import _lib, brush_project_main, build, config as cfgmod, formats, painting, projection, weights as wmod

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("nb_projection_masks_f32", "nb_projection_loss_f32", "nb_projection_loss_bwd_f32")
t = torch.from_numpy
opt = lambda x: None if x is None else t(x)


@pytest.fixture(scope="module")
def gold():
    return load_golden("projection.npz")


@pytest.fixture(scope="module")
def ex(gold):
    """The exemplar of the golden runs: (target [B,3,32,32], geom [B,1,32,32], None, None)."""
    e = pr.exemplar(32, int(gold["patches"]), seed=int(gold["exemplar_seed"]))
    assert float(e[0].double().sum()) == float(gold["target_sum"]) and float(e[1].double().sum()) == float(gold["geom_sum"])
    return e


@pytest.fixture(scope="module")
def tiny(gold):
    cfg = cfgmod.tiny_config(32)
    return cfg, wmod.random_state_dict(cfg, seed=int(gold["state_seed"]))


def _masks_of(c):
    m = t(c["mask"].astype(np.int64)).unsqueeze(1)
    return ((m >> 1) & 1).bool(), (m & 1).bool()


VARIANTS = [(True, False), (True, True), (False, False)]                   # (composite, bg_image)


# ------------------------------------------------------------------------------------------------
# the statement against its own autograd and central differences
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("composite,bg_image", VARIANTS)
def test_statement_gradients_equal_float64_autograd(composite, bg_image):
    c = pr.loss_case(20, 3, 2, composite=composite, bg_image=bg_image, no_fg_patch=True)
    w, k = c["weights"], 2
    uvs, colors, img = (t(c[n]).double().requires_grad_(True) for n in ("uvs", "colors", "img"))
    gscale = torch.tensor([1.0, 0.25], dtype=torch.float64)
    d_synth = t(np.random.RandomState(1).randn(*c["uvs"].shape)) * 1e-3
    out, synth = pr.loss_f64(uvs, colors, img, c["target"], c["bg_image"], c["bg_color"], c["mask"], k, composite, w)
    ((out[:, 2] * gscale).sum() + (synth * d_synth).sum()).backward()
    du, di, dc = pr.loss_bwd_f64(c["uvs"], c["colors"], c["img"], c["target"], c["bg_image"], c["bg_color"], c["mask"], k, composite, w, d_synth, gscale)
    if composite:
        assert np.abs(du - uvs.grad.numpy()).max() <= 1e-14 * max(1.0, np.abs(du).max())
        assert np.abs(dc - colors.grad.numpy()).max() <= 1e-13 * max(1.0, np.abs(dc).max())
        assert img.grad is None and di is None
    else:
        assert np.abs(du - uvs.grad.numpy()).max() <= 1e-15 and np.all(du[:, :2] == 0) and colors.grad is None and dc is None
        assert np.abs(di - img.grad.numpy()).max() <= 1e-15


def test_statement_backward_against_central_differences():
    """Away from the kinks of |.|: the loss is linear in colors and bilinear in uvs, so a central difference with h = 1e-6 in float64 is
    exact to rounding (~1e-10 relative) wherever no |target - synth| changes sign within h."""
    c = pr.loss_case(8, 2, 1, composite=True, bg_image=False, seed=3)
    w, rs, h = c["weights"], np.random.RandomState(0), 1e-6
    f = lambda uvs, colors: float(pr.loss_f64(uvs, colors, None, c["target"], None, c["bg_color"], c["mask"], 1, True, w)[0][0, 2])
    du, _, dc = pr.loss_bwd_f64(c["uvs"], c["colors"], None, c["target"], None, c["bg_color"], c["mask"], 1, True, w)
    u0, c0 = c["uvs"].astype(np.float64), c["colors"].astype(np.float64)
    for _ in range(12):
        i = tuple(rs.randint(0, s) for s in u0.shape)
        if i[2] < 4 and i[3] < 2:                                          # the sign-0 region: a kink by construction
            continue
        up, um = u0.copy(), u0.copy()
        up[i] += h
        um[i] -= h
        assert (f(up, c0) - f(um, c0)) / (2 * h) == pytest.approx(du[i], rel=1e-6, abs=1e-9), i
    for i in np.ndindex(2, 3, 3):
        cp, cm = c0.copy(), c0.copy()
        cp[i] += h
        cm[i] -= h
        assert (f(u0, cp) - f(u0, cm)) / (2 * h) == pytest.approx(dc[i], rel=1e-6, abs=1e-9), i


# ------------------------------------------------------------------------------------------------
# route "torch" against the statement
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("composite,bg_image", VARIANTS)
@pytest.mark.parametrize("r,b,k", [(8, 1, 1), (20, 3, 2), (64, 3, 1)])
def test_torch_loss_against_statement(r, b, k, composite, bg_image):
    """Bound: ``clarity_refs.bound`` with no measured part (the route IS the float32 side), that is ULP_FLOOR ulps -- of the largest
    value, times 8: a float32 mean over up to 3 * 3 * 64 * 64 terms in pairwise order carries log2(n) ~ 17 roundings, and the
    composite four more."""
    c = pr.loss_case(r, b, k, composite=composite, bg_image=bg_image, no_fg_patch=b > 1)
    fg, bg = _masks_of(c)
    w = c["weights"]
    uvs, colors, img = (t(c[n]).requires_grad_(True) for n in ("uvs", "colors", "img"))
    out, synth = projection.loss_torch(uvs, colors, img, t(c["target"]), opt(c["bg_image"]), t(c["bg_color"]), fg, bg, k, composite, w)
    out[:, 2].sum().backward()
    out64, synth64 = pr.loss_f64(c["uvs"], c["colors"], c["img"], c["target"], c["bg_image"], c["bg_color"], c["mask"], k, composite, w)
    du, di, dc = pr.loss_bwd_f64(c["uvs"], c["colors"], c["img"], c["target"], c["bg_image"], c["bg_color"], c["mask"], k, composite, w)
    tol = lambda ref: 8 * cr.bound(ref, ref, value=np.abs(ref).max()) + 1e-30
    assert np.all(np.abs(out.detach().numpy() - out64.numpy()) <= tol(out64.numpy()))
    assert np.all(np.abs(synth.detach().numpy() - synth64.numpy()) <= tol(synth64.numpy()))
    assert np.all(np.abs(uvs.grad.numpy() - du) <= tol(du))
    if composite:
        assert np.all(np.abs(colors.grad.numpy() - dc) <= tol(dc))
    else:
        assert np.all(np.abs(img.grad.numpy() - di) <= tol(di))
    # in float64 the route is the statement
    out_d, _ = projection.loss_torch(t(c["uvs"]).double(), t(c["colors"]).double(), t(c["img"]).double(), t(c["target"]).double(),
                                     None if c["bg_image"] is None else t(c["bg_image"]).double(), t(c["bg_color"]).double(), fg, bg, k, composite, w)
    assert np.abs(out_d.numpy() - out64.numpy()).max() <= 1e-14


def test_torch_masks_against_statement():
    for r, k, b in ((32, 2, 2), (64, 1, 3)):
        geom = t(pr.drawings(r, k * b, seed=r))
        target = torch.rand(k * b, 3, r, r, generator=torch.Generator().manual_seed(r)) * 2 - 1
        mask64, counts64, color64 = pr.masks_f64(geom, target, k)
        fg, bg = projection.conservative_masks_torch(geom)
        assert np.array_equal(fg[:, 0].numpy(), (mask64 >> 1) & 1) and np.array_equal(bg[:, 0].numpy(), mask64 & 1)
        assert counts64.min() >= 37                                        # (every exemplar has both kinds of pixels)
        color = projection.masked_color_torch(target, bg, k).numpy()
        assert np.abs(color - color64).max() <= 8 * cr.EPS32
    # an exemplar without background: zeros
    z = projection.masked_color_torch(torch.ones(1, 3, 8, 8), torch.zeros(1, 1, 8, 8, dtype=torch.bool), 1)
    assert torch.equal(z, torch.zeros(1, 3))


# ------------------------------------------------------------------------------------------------
# the projector, route "torch", on the oracle
# ------------------------------------------------------------------------------------------------
def _projector(gold, tiny, draws=None, **kw):
    cfg, sd = tiny
    kw.setdefault("l1_fg_weight", float(gold["weights"][0]))
    kw.setdefault("bg_weight", float(gold["weights"][1]))
    kw.setdefault("num_steps", int(gold["num_steps"]))
    return projection.BrushProjector(pr.OracleGen(cfg, sd), cr.StandInEncoder(cfg), route="torch", w_avg=gold["w_avg"], w_std=float(gold["w_std"]),
                                     draws=draws, **kw)


@pytest.mark.parametrize("run,w_plus,composite", [("wplus_comp", True, True), ("w_nocomp", False, False)])
def test_projector_reproduces_the_reference_run(gold, tiny, ex, run, w_plus, composite):
    """The rule of test_clarity_cpu.py for clarity_opt.npz.  Bound: eps_ref x FACTOR, FACTOR = sum_t 2 lr_t / min sqrt(v_hat_t) with the
    smallest Adam denominators of the float64 run of this case: an error d in a gradient moves Adam's update by at most
    2 lr d / sqrt(v_hat).  On the CPU the reference returns the state after its last step (its 'best' tensors alias the live ones), so
    the projector's ``last_rows`` are compared."""
    n = int(gold["num_steps"])
    draws = cr.ReplayDraws(gold["init_noise"], gold[f"{run}/w_noise"][:, None], np.zeros([n, 1], np.int64))
    p = _projector(gold, tiny, draws, w_plus=w_plus, with_composite=composite, perceptual=pr.stand_in_perceptual)
    rec = []
    out = p.project({"a": (ex[0], ex[1], None, None)},
                    on_step=lambda ids, s, lr, items, reg: rec.append((lr, items.numpy().copy())))
    eps = float(gold[f"{run}/eps_ref"])
    factor = float(np.sum(2 * gold[f"{run}/lr"] / gold[f"{run}/adam_denom_min"]))
    assert factor >= 1 and eps <= float(gold["eps_ref"])
    ref_row = np.concatenate([gold[f"{run}/final_w"].reshape(-1), gold[f"{run}/final_noise"]])
    e_row = np.abs(p.last_rows["a"].numpy() - ref_row).max()
    perc = np.array([r[1][0, p.item_names.index("perceptual")] for r in rec])
    e_perc = np.abs(perc - gold[f"{run}/perceptual"]).max()
    e_bg = np.abs(out["a"]["bg"].numpy() - gold[f"{run}/bg"]).max()
    print(f"[projection] {run}: torch route vs reference: final {e_row:.3g}, perceptual {e_perc:.3g}, bg {e_bg:.3g}; bound {eps * factor:.3g} "
          f"(eps_ref {eps:.3g} x {factor:.3g})")
    assert e_row <= eps * factor and e_perc <= eps * factor and e_bg <= eps * factor
    assert np.array_equal(np.array([r[0] for r in rec]), gold[f"{run}/lr"])
    # the result: the row of the step with the lowest perceptual value, the reference's shapes
    cfg = tiny[0]
    assert out["a"]["w"].shape == (1, cfg.num_ws if w_plus else 1, cfg.w_dim) and out["a"]["step"] == n - 1 and out["a"]["bg"].shape == (3,)
    assert sorted(out["a"]["noise"]) == sorted(p.layout.names) and set(p.history["a"]) == {"first", "last"}
    assert p.history["a"]["first"]["perceptual"] == pytest.approx(gold[f"{run}/perceptual"][0], abs=1e-5)


def test_a_brush_alone_and_in_a_pass_of_two(gold, tiny, ex):
    exs = {"a": (ex[0], ex[1], None, None), "b": pr.exemplar(32, ex[1].shape[0], seed=23)}
    runs = {}
    for name, per_pass in (("together", 2), ("alone", 1)):
        p = _projector(gold, tiny, w_plus=True, with_composite=True, num_steps=4)
        runs[name] = p.project(exs, brushes_per_pass=per_pass, seed=5)
    eps = float(gold["eps_ref"])
    for sid in ("a", "b"):
        a, b = runs["together"][sid], runs["alone"][sid]
        assert float((a["w"] - b["w"]).abs().max()) <= eps and torch.equal(a["bg"], b["bg"]) and a["step"] == b["step"]
        for n in a["noise"]:
            assert float((a["noise"][n] - b["noise"][n]).abs().max()) <= eps, (sid, n)
    assert float((runs["alone"]["a"]["noise"]["b4.conv1.noise_const"] - runs["alone"]["b"]["noise"]["b4.conv1.noise_const"]).abs().max()) > 1e-2


def test_best_state_and_early_stop_on_a_scripted_criterion(gold, tiny, ex, monkeypatch):
    """The perceptual plug returns scripted values: brush 0 improves until step 2 and then worsens, brush 1 keeps improving.  With a
    check every 2 steps brush 0 is finished at the check of step 4 (nothing gained since step 2), brush 1 runs to the end."""
    monkeypatch.setattr(projection, "CHECK_EVERY", 2)
    script = {0: [5.0, 4.0, 3.0, 3.5, 3.6, 3.7, 3.8, 3.9], 1: [5.0, 4.5, 4.0, 3.5, 3.0, 2.5, 2.0, 1.5]}
    calls, b = [], ex[1].shape[0]

    def scripted(target, synth):
        s = len(calls)
        calls.append(s)
        vals = torch.tensor([script[i][s] for i in range(2) for _ in range(b)], dtype=synth.dtype)
        return vals + 0 * synth.mean(dim=(1, 2, 3))

    p = _projector(gold, tiny, w_plus=False, with_composite=False, perceptual=scripted, num_steps=8, min_improvement=0.01)
    arenas = []
    orig = p.loss_and_grad
    monkeypatch.setattr(p, "loss_and_grad", lambda arena, *a, **k: (arenas.append(arena.clone()), orig(arena, *a, **k))[1])
    out = p.project({"x": (ex[0], ex[1], None, None), "y": pr.exemplar(32, b, seed=23)}, brushes_per_pass=2, seed=1)
    assert out["x"]["step"] == 4 and out["y"]["step"] == 7 and len(calls) == 8
    # 'last' is the step a brush finished at, not the pass's last step
    assert p.history["x"]["last"]["perceptual"] == pytest.approx(3.6) and p.history["y"]["last"]["perceptual"] == pytest.approx(1.5)
    assert p.history["x"]["first"]["perceptual"] == p.history["y"]["first"]["perceptual"] == pytest.approx(5.0)
    lo = p.layout
    assert torch.equal(out["x"]["w"], lo.w(arenas[2])[0:1]) and torch.equal(out["y"]["w"], lo.w(arenas[7])[1:2])
    assert torch.equal(out["x"]["noise"]["b8.conv0.noise_const"], lo.plane(arenas[2], lo.names.index("b8.conv0.noise_const"))[0])
    # all brushes finished: the pass ends at that check
    del calls[:]
    script[1] = script[0]
    out = p.project({"x": (ex[0], ex[1], None, None), "y": pr.exemplar(32, b, seed=23)}, brushes_per_pass=2, seed=1)
    assert out["x"]["step"] == out["y"]["step"] == 4 and len(calls) == 5


def test_options_and_errors(gold, tiny, ex):
    cfg, sd = tiny
    gen, enc = pr.OracleGen(cfg, sd), cr.StandInEncoder(cfg)
    with pytest.raises(ValueError, match="at least one of l1_fg_weight, bg_weight"):
        projection.BrushProjector(gen, enc, route="torch")
    with pytest.raises(ValueError, match="route"):
        projection.BrushProjector(gen, enc, route="cuda", l1_fg_weight=1)
    with pytest.raises(_lib.NeubeHipError, match="needs a GPU"):
        projection.BrushProjector(gen, enc, route="hip", l1_fg_weight=1, device="cpu")
    target, geom = ex[0], ex[1]
    p = _projector(gold, tiny, num_steps=2)
    with pytest.raises(ValueError, match="'white'.*foreground"):
        p.project({"white": (target, torch.ones_like(geom), None, None)})
    p = _projector(gold, tiny, num_steps=2, l1_fg_weight=1.0, bg_weight=0.0, with_composite=True)
    with pytest.raises(ValueError, match="'black'.*background"):
        p.project({"black": (target, torch.zeros_like(geom), None, None)})
    out = p.project({"black": (target, torch.zeros_like(geom), None, target)})           # a background image: no mean colour needed
    assert torch.equal(out["black"]["bg"], torch.zeros(3))
    with pytest.raises(ValueError, match="with_positions"):
        _projector(gold, tiny, num_steps=1, with_positions=True).project({"a": (target, geom, None, None)})
    with pytest.raises(ValueError, match="an exemplar is"):
        p.project({"a": (target[:, :, :16], geom, None, None)})
    # W only, no planes: the generator's own noise_const; resume_from supplies W
    w0 = torch.randn(1, 1, cfg.w_dim, generator=torch.Generator().manual_seed(0))
    p = _projector(gold, tiny, num_steps=1, w_plus=False, optimize_noise=False, resume_from={"a": {"w": w0, "noise": {"ignored": 1}}})
    out = p.project({"a": (target, geom, t(np.zeros([3, 2], np.float32)), None)}, seed=0)
    assert out["a"]["noise"] == {} and p.layout.p == cfg.w_dim and torch.equal(out["a"]["w"], w0)
    p = _projector(gold, tiny, num_steps=1, w_plus=True, resume_from={"a": {"w": w0}})
    assert torch.equal(p.project({"a": (target, geom, None, None)}, seed=0)["a"]["w"], w0.expand(1, cfg.num_ws, cfg.w_dim))


def test_map_style_repeats_a_one_row_w(tiny):
    """``TileOps.map_style``: a brush projected into W ([N,1,w_dim]) is repeated over num_ws (project_main.py:460); W+ passes as it is."""
    import types
    cfg = tiny[0]
    ops = types.SimpleNamespace(device=torch.device("cpu"), cfg=cfg)
    g = torch.Generator().manual_seed(0)
    w1, wp = torch.randn(2, 1, cfg.w_dim, generator=g), torch.randn(2, cfg.num_ws, cfg.w_dim, generator=g)
    got = painting.TileOps.map_style(ops, ws=w1)
    assert cfg.num_ws > 1 and got.shape == (2, cfg.num_ws, cfg.w_dim) and got.is_contiguous() and torch.equal(got, w1.expand(2, cfg.num_ws, cfg.w_dim))
    assert torch.equal(painting.TileOps.map_style(ops, ws=wp), wp)
    assert painting.TileOps.map_style(ops, ws=wp.double()).dtype == torch.float32


# ------------------------------------------------------------------------------------------------
# samplers
# ------------------------------------------------------------------------------------------------
def _exemplar_image(h=120, w=160, seed=0):
    rs = np.random.RandomState(seed)
    geom = np.full([h, w, 3], 255, np.uint8)
    geom[40:70, 20:140] = 0
    target = rs.randint(0, 256, [h, w, 4]).astype(np.uint8)
    return target, geom, rs.randint(0, 256, [h, w, 3]).astype(np.uint8)


def test_load_target_boxes_and_positions():
    target, geom, _ = _exemplar_image()
    a = projection.load_target(target, geom, 32, crop_n=6, patch_range=(0.2, 0.5), rng=np.random.default_rng(4), return_boxes=True)
    b = projection.load_target(target, geom, 32, crop_n=6, patch_range=(0.2, 0.5), rng=np.random.default_rng(4), return_boxes=True)
    c = projection.load_target(target, geom, 32, crop_n=6, patch_range=(0.2, 0.5), rng=np.random.default_rng(5), return_boxes=True)
    assert a[3] == b[3] and a[3] != c[3] and all(torch.equal(x, y) for x, y in zip(a[:3], b[:3]))
    tp, gp, pos, boxes = a
    assert tp.shape == (6, 3, 32, 32) and gp.shape == (6, 1, 32, 32) and pos.shape == (6, 2) and tp.dtype == torch.float32
    assert 0 <= float(tp.min()) and float(tp.max()) <= 1 and 0 <= float(gp.min()) and float(gp.max()) <= 1
    for col, row, rw, rh in boxes:
        assert rw == rh and int(0.2 * 120) <= rw <= int(0.5 * 120) and 0 <= col <= 160 - rw and 0 <= row <= 120 - rw
    want = torch.tensor([x[:2] for x in boxes]) * 32 / (0.2 * 120)                          # project_main.py:342-343
    assert torch.equal(pos, want)
    # a box that is exactly a multiple of the patch: the resize is then a box filter
    one = projection._fixed_patch(np.repeat(np.arange(64, dtype=np.float32)[None, :, None], 64, 0), 0, 0, 64, 64, 32)
    assert np.abs(one[0, :, 0] - (np.arange(32) * 2 + 0.5)).max() <= 0.3
    # overfit_one: shifted copies of one box, then the transposed patches
    tp, gp, pos, boxes = projection.load_target(target, geom, 32, crop_n=10, rng=np.random.default_rng(1), overfit_one=True, return_boxes=True)
    n = len(boxes)
    assert n == 3 and tp.shape[0] == 2 * n and len({(bx[0], bx[2]) for bx in boxes}) == 1
    assert torch.equal(tp[n:], tp[:n].permute(0, 1, 3, 2)) and torch.equal(gp[n:], gp[:n].permute(0, 1, 3, 2)) and torch.equal(pos[n:], pos[:n])
    with pytest.raises(ValueError, match="geometry image"):
        projection.load_target(target, geom[:50], 32)
    with pytest.raises(NotImplementedError):
        projection.load_target(target[:32, :32], geom[:32, :32], 32)


def test_load_target_sparse_boxes_positions_and_bound():
    target, geom, bgimg = _exemplar_image()
    a = projection.load_target_sparse(target, bgimg, geom, 32, crop_n=5, rng=np.random.default_rng(2), return_boxes=True)
    b = projection.load_target_sparse(target, bgimg, geom, 32, crop_n=5, rng=np.random.default_rng(2), return_boxes=True)
    assert a[4] == b[4] and all(torch.equal(x, y) for x, y in zip(a[:4], b[:4]))
    tp, bp, gp, pos, boxes = a
    assert tp.shape == bp.shape == (5, 3, 32, 32) and gp.shape == (5, 1, 32, 32)
    assert torch.equal(pos, torch.tensor([x[:2] for x in boxes]) * 32 / (0.2 * 120))        # project_main.py:288-289
    g = geom[..., 1].astype(np.float32) / 255
    for col, row, rw, _ in boxes:
        assert np.sum(g[row:row + rw, col:col + rw] < 0.1) > rw * rw * 0.05
    # where the drawing is stroke the background patches are the background image, elsewhere the exemplar
    full = projection.load_target_sparse(target, bgimg, geom, 32, crop_n=1, patch_range=(1.0, 1.0), rng=np.random.default_rng(0))
    assert full[1].shape == (1, 3, 32, 32) and not torch.equal(full[0], full[1])
    assert projection.load_target_sparse(target, None, geom, 32, crop_n=2, rng=np.random.default_rng(0))[1] is None
    # the retry loop is bounded: a drawing with a single stroke pixel cannot fill 5% of any box
    thin = np.full_like(geom, 255)
    thin[60, 80] = 0
    with pytest.raises(ValueError, match="of 3 boxes"):
        projection.load_target_sparse(target, None, thin, 32, crop_n=3, rng=np.random.default_rng(0))


# ------------------------------------------------------------------------------------------------
# command line
# ------------------------------------------------------------------------------------------------
def test_cli_end_to_end_with_patches(gold, tiny, ex, tmp_path, capsys):
    cfg, sd = tiny
    patches = tmp_path / "oil.npz"
    np.savez(patches, target=ex[0].numpy(), geom=ex[1].numpy(), positions=np.arange(6, dtype=np.float32).reshape(3, 2))
    engine = (pr.OracleGen(cfg, sd), cr.StandInEncoder(cfg), torch.device("cpu"))
    argv = ["--gan_checkpoint", "unused.npz", "--output_dir", str(tmp_path / "out"), "--patches", str(patches), "--num_steps", "3", "--w_plus",
            "--with_composite", "--with_positions", "--l1_fg_weight", "1.0", "--bg_weight", "0.5", "--seed", "3", "--num_crops", "3"]
    pkl, info = brush_project_main.main(argv, engine=engine)
    assert os.path.basename(pkl) == "ALL_projected_wplus_optnoise_ncrop3.pkl" and os.path.basename(info) == "projection.json"
    lib = formats.WBrushLibrary.from_file(pkl, strict=True)
    assert lib.get_style_ids() == ["oil"]
    opts = painting.GanBrushOptions()
    lib.set_style("oil", opts)
    assert opts.style_ws.shape == (1, cfg.num_ws, cfg.w_dim)
    bufs = opts.custom_args["noise_buffers"]
    assert sorted(bufs) == sorted(l.name[len("synthesis."):] + ".noise_const" for l in cfg.layers) and bufs["b32.conv1.noise_const"].shape == (32, 32)
    with open(info) as f:
        j = json.load(f)
    assert set(j["oil"]) == {"first", "last", "step", "bg"} and set(j["oil"]["first"]) == {"l1", "bg", "noise_reg"} and j["oil"]["step"] == 2
    with np.load(str(tmp_path / "out" / "oil_projected_wplus_optnoise_ncrop3.npz")) as z:
        assert z["w"].shape == (1, cfg.num_ws, cfg.w_dim) and "b4.conv1.noise_const" in z.files and z["bg"].shape == (3,)
    # --skip_existing: nothing to do; --resume with another id: skipped as well
    assert brush_project_main.main(argv + ["--skip_existing"], engine=engine) == (pkl, None)
    assert brush_project_main.main(argv + ["--resume", "--output_style_id", "other"], engine=engine) == (pkl, None)
    # the parser: the reference's arguments and defaults
    a = brush_project_main.build_parser().parse_args(["--gan_checkpoint", "e.npz", "--output_dir", "o", "--target_image", "a.png", "--geom_image", "ag.png",
                                                      "--target_image", "b.png", "--geom_image", "bg.png"])
    assert (a.num_steps, a.num_crops, a.patch_scale_range, a.l1_fg_weight, a.bg_weight, a.brushes_per_pass) == (1000, 10, (0.2, 0.5), 0, 0, 4)
    assert a.target_image == ["a.png", "b.png"] and not (a.w_plus or a.no_noise or a.with_positions or a.overfit_one or a.with_composite or a.resume)
    assert brush_project_main.file_suffix(a) == "w_optnoise_ncrop10"
    with pytest.raises(SystemExit):
        brush_project_main.build_parser().parse_args(["--gan_checkpoint", "e.npz", "--output_dir", "o", "--patch_scale_range", "0.6,0.5"])


def test_cli_reads_images_through_the_samplers(gold, tiny, tmp_path):
    from PIL import Image
    cfg, sd = tiny
    target, geom, _ = _exemplar_image()
    for name, arr in (("chalk.png", target[..., :3]), ("chalk_geom.png", geom), ("ink.png", target[::-1, :, :3].copy()), ("ink_geom.png", geom[::-1].copy())):
        Image.fromarray(arr).save(tmp_path / name)
    argv = ["--gan_checkpoint", "unused.npz", "--output_dir", str(tmp_path / "out"), "--num_steps", "1", "--l1_fg_weight", "1.0", "--seed", "1", "--num_crops", "2",
            "--patch_scale_range", "0.4,0.6", "--brushes_per_pass", "2"]
    for n in ("chalk", "ink"):
        argv += ["--target_image", str(tmp_path / f"{n}.png"), "--geom_image", str(tmp_path / f"{n}_geom.png")]
    pkl, _ = brush_project_main.main(argv, engine=(pr.OracleGen(cfg, sd), cr.StandInEncoder(cfg), torch.device("cpu")))
    lib = formats.WBrushLibrary.from_file(pkl)
    assert lib.get_style_ids() == ["chalk", "ink"] and lib.styles["ink"]["w"].shape == (1, 1, cfg.w_dim)


# ------------------------------------------------------------------------------------------------
# the C entries: host-side argument checks, header, build
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def library():
    build.build()
    return _lib.lib()


def test_entry_argument_checks(library):
    err = lambda: library.nb_last_error().decode()
    P = 0x1000                                                             # never dereferenced: the checks come before any HIP call
    masks = lambda blur=P, target=P, stride=192, k=1, b=1, r=8, mask=P, counts=P: library.nb_projection_masks_f32(blur, target, stride, k, b, r, mask, counts,
                                                                                                              P, P, None)
    assert masks(blur=None) == _lib.NB_EINVAL and "null pointer" in err()
    assert masks(mask=None) == _lib.NB_EINVAL and "null pointer" in err()
    assert masks(k=-1) == _lib.NB_EINVAL and "bad sizes" in err()
    assert masks(b=0) == _lib.NB_EINVAL and "bad sizes" in err()
    assert masks(r=4097) == _lib.NB_EINVAL and "r in 1..4096" in err()
    assert masks(k=4096, b=16) == _lib.NB_EINVAL and "k * b <= 65535" in err()
    assert masks(stride=191) == _lib.NB_EINVAL and "stride" in err()
    assert masks(target=P + 2) == _lib.NB_EINVAL and "aligned" in err()
    assert masks(counts=P + 1) == _lib.NB_EINVAL and "aligned" in err()
    assert masks(k=0) == _lib.NB_OK

    def loss(uvs=P, us=192, colors=P, img=None, is_=0, target=P, ts=192, bgi=None, bs=0, bgc=P, mask=P, counts=P, k=1, b=1, r=8, comp=1, synth=P, out=P,
             partials=P):
        return library.nb_projection_loss_f32(uvs, us, colors, img, is_, target, ts, bgi, bs, bgc, mask, counts, k, b, r, comp, 1.0, 1.0, synth, out, partials, None)
    assert loss(uvs=None) == _lib.NB_EINVAL and "null pointer" in err()
    assert loss(colors=None) == _lib.NB_EINVAL and "composite needs colors" in err()
    assert loss(bgc=None) == _lib.NB_EINVAL and "one of bg_image, bg_color" in err()
    assert loss(synth=None) == _lib.NB_EINVAL and "synth with composite" in err()
    assert loss(comp=0) == _lib.NB_EINVAL and "no composite needs img" in err()
    assert loss(b=0) == _lib.NB_EINVAL and "bad sizes" in err()
    assert loss(us=191) == _lib.NB_EINVAL and "stride" in err()
    assert loss(bgi=P, bs=100) == _lib.NB_EINVAL and "stride" in err()
    assert loss(comp=0, img=P, is_=10) == _lib.NB_EINVAL and "stride" in err()
    assert loss(target=P + 1) == _lib.NB_EINVAL and "aligned" in err()
    assert loss(out=P + 2) == _lib.NB_EINVAL and "aligned" in err()
    assert loss(k=0) == _lib.NB_OK
    assert loss(k=0, comp=0, img=P, is_=192, colors=None, bgc=None, synth=None) == _lib.NB_OK      # the optional ones
    assert loss(k=0, bgi=P, bs=192, bgc=None) == _lib.NB_OK

    def bwd(uvs=P, colors=P, img=None, is_=0, ts=192, bgi=None, bs=0, bgc=P, counts=P, d_synth=None, gscale=None, k=1, b=1, r=8, comp=1, d_uvs=P, d_img=None,
            d_colors=P, partials=P):
        return library.nb_projection_loss_bwd_f32(uvs, 192, colors, img, is_, P, ts, bgi, bs, bgc, P, counts, d_synth, gscale, k, b, r, comp, 1.0, 1.0, d_uvs,
                                                  d_img, d_colors, partials, None)
    assert bwd(counts=None) == _lib.NB_EINVAL and "null pointer" in err()
    assert bwd(d_uvs=None) == _lib.NB_EINVAL and "null pointer" in err()
    assert bwd(d_colors=None) == _lib.NB_EINVAL and "d_colors and partials with composite" in err()
    assert bwd(comp=0, img=P, is_=192) == _lib.NB_EINVAL and "d_img without" in err()
    assert bwd(ts=10) == _lib.NB_EINVAL and "stride" in err()
    assert bwd(r=0) == _lib.NB_EINVAL and "bad sizes" in err()
    assert bwd(gscale=P + 2) == _lib.NB_EINVAL and "aligned" in err()
    assert bwd(d_synth=P + 1) == _lib.NB_EINVAL and "aligned" in err()
    assert bwd(k=0) == _lib.NB_OK and bwd(k=0, d_synth=P, gscale=P) == _lib.NB_OK
    assert bwd(k=0, comp=0, img=P, is_=192, d_img=P, colors=None, bgc=None, d_colors=None, partials=None) == _lib.NB_OK


def test_header_abi_version_and_sources(library):
    text = open(os.path.join(REPO, "include", "neube_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
        assert name in _lib.PROTOTYPES and hasattr(library, name)
    assert "project_main.py:248-250" in text and "geom_metric.py:132-140" in text and "visualize.py:315-323" in text
    assert re.search(r"#define NB_ABI_VERSION 22\b", open(os.path.join(build.CSRC, "nb_common.h")).read())
    assert _lib.ABI_VERSION == 22 and library.nb_abi_version() == 22
    assert "nb_projection.hip" in build.SOURCES and build.FILE_FLAGS["nb_projection.hip"] == ["-fno-slp-vectorize"]
    assert re.search(rf"#define NB_PROJECTION_PARTS {_lib.NB_PROJECTION_PARTS}\b", text)
    res = {k: v for k, v in build.kernel_resources().items() if "projection_" in k}
    assert len(res) >= 12 and not any(v["scratch_bytes"] or v["vgpr_spill"] for v in res.values()), res
