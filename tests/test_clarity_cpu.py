"""CPU: the clarity optimisation (brushstroke_engine_amd/clarity.py) against the reference's run_one_clarity_opt recorded in
tests/golden/clarity_opt.npz (tests/golden/make_golden_clarity.py) and against the float64 statement of tests/clarity_refs.py; the
C entries' argument checks (host code: no GPU needed); the command line's files."""
import ctypes as C
import json
import os
import pickle
import re

import numpy as np
import pytest
import torch

import clarity_refs as cr
from conftest import load_golden
from brushstroke_engine_amd import _lib, brush_clarity_main, build, clarity, config as cfgmod, formats, painting, weights as wmod

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("nb_clarity_loss_f32", "nb_clarity_loss_bwd_f32", "nb_noise_reg_f32", "nb_clarity_step_f32")


@pytest.fixture(scope="module")
def gold():
    return load_golden("clarity_opt.npz")


@pytest.fixture(scope="module")
def tiny(gold):
    cfg = cfgmod.tiny_config(32)
    sd = wmod.random_state_dict(cfg, seed=int(gold["state_seed"]))
    return cfg, sd


def _golden_order(gold, names):
    have = [str(n) for n in gold["item_names"]]
    return [have.index(n) for n in names]


# ------------------------------------------------------------------------------------------------
# the statement against the reference run, and against its own autograd
# ------------------------------------------------------------------------------------------------
def test_statement_reproduces_the_reference_run(gold, tiny):
    cfg, sd = tiny
    draws = cr.ReplayDraws(gold["init_noise"], gold["w_noise"], gold["drawing_idx"])
    steps, row = cr.run_statement_loop(cr.OracleGen(cfg, sd, torch.float64), cr.StandInEncoder(cfg), gold["drawings"], torch.from_numpy(gold["w_start"]),
                                       draws, int(gold["num_steps"]), int(gold["batch"]), float(gold["w_std"]))
    eps = float(gold["eps_ref"])
    items = np.array([s[1] for s in steps])[:, [["iou_inv_uvs", "iou_u", "l1_fake_orig"].index(str(n)) for n in gold["item_names"]]]
    ref_row = np.concatenate([gold["final_w"].reshape(-1), gold["final_noise"]])
    print(f"[clarity] statement vs reference: items {np.abs(items - gold['items']).max():.3g}, final {np.abs(row - ref_row).max():.3g}, eps_ref {eps:.3g}")
    assert np.abs(items - gold["items"]).max() <= eps and np.abs(row - ref_row).max() <= eps
    assert np.abs(np.array([s[2] for s in steps]) - gold["reg_ref_states"]).max() <= eps
    assert np.array_equal(np.array([s[0] for s in steps]), gold["lr"])


def test_statement_gradients_equal_float64_autograd():
    c = cr.loss_case(20, 3, 2)
    w = c["weights"]
    uvs, img = torch.from_numpy(c["uvs"]).double().requires_grad_(True), torch.from_numpy(c["img"]).double().requires_grad_(True)
    gscale = torch.tensor([1.0, 0.25], dtype=torch.float64)
    out, sums = cr.loss_f64(uvs, img, torch.from_numpy(c["target"]).double(), torch.from_numpy(c["geom"]).double(), 2, w)
    (out[:, 3] * gscale).sum().backward()
    du, di = cr.loss_bwd_f64(c["img"], c["target"], c["geom"], sums, 2, w, gscale.numpy())
    assert np.abs(du - uvs.grad.numpy()).max() <= 1e-15 * max(1.0, np.abs(du).max()) and np.array_equal(di, img.grad.numpy())
    lo = cr.reg_layout()
    a = torch.from_numpy(cr.reg_arena(2)).double().requires_grad_(True)
    cr.noise_reg_f64(a, lo).sum().backward()
    g = cr.noise_reg_grad_f64(a, lo)
    assert np.abs(g - a.grad.numpy()).max() <= 1e-15 * np.abs(g).max() and np.abs(g[:, lo.nw:]).min() >= 0 and np.all(g[:, :lo.nw] == 0)
    # the step against torch.optim.Adam in float64, t = 1, 2, 3 from zero state
    rs = np.random.RandomState(0)
    x = torch.from_numpy(cr.reg_arena(1).astype(np.float64)).requires_grad_(True)
    adam = torch.optim.Adam([x], betas=(0.9, 0.999), lr=0.03)
    arena, m, v = x.detach().numpy().copy(), np.zeros([1, lo.p]), np.zeros([1, lo.p])
    for t in (1, 2, 3):
        grad = rs.randn(1, lo.p) * 1e-3
        x.grad = torch.from_numpy(grad.copy())
        adam.step()
        with torch.no_grad():
            for i in range(len(lo.res)):
                buf = lo.plane(x, i)
                buf -= buf.mean()
                buf *= buf.square().mean().rsqrt()
        arena, m, v = cr.step_f64(arena, grad, m, v, lo, 0.03, t)
        assert np.abs(arena - x.detach().numpy()).max() <= 1e-13, t


# ------------------------------------------------------------------------------------------------
# route "torch" against the statement
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r,b,k", cr.LOSS_CASES, ids=[f"r{r}_b{b}_k{k}" for r, b, k in cr.LOSS_CASES])
def test_torch_loss_against_statement(r, b, k):
    c = cr.loss_case(r, b, k)
    t = lambda x: torch.from_numpy(x)
    uvs, img = t(c["uvs"]).requires_grad_(True), t(c["img"]).requires_grad_(True)
    out = clarity.loss_torch(uvs, img, t(c["target"]), t(c["geom"]), k, c["weights"])
    out[:, 3].sum().backward()
    out64, sums64 = cr.loss_f64(c["uvs"], c["img"], c["target"], c["geom"], k, c["weights"])
    du, di = cr.loss_bwd_f64(c["img"], c["target"], c["geom"], sums64, k, c["weights"])
    assert np.abs(out.detach().numpy() - out64.numpy()).max() <= 32 * cr.EPS32 * np.abs(out64.numpy()).max()
    assert np.abs(uvs.grad.numpy() - du).max() <= 32 * cr.EPS32 * np.abs(du).max() + 1e-30
    assert np.abs(img.grad.numpy() - di).max() <= 4 * cr.EPS32 * np.abs(di).max()
    # in float64 the route is the statement
    out_d = clarity.loss_torch(t(c["uvs"]).double(), t(c["img"]).double(), t(c["target"]).double(), t(c["geom"]).double(), k, c["weights"])
    assert np.abs(out_d.numpy() - out64.numpy()).max() <= 1e-14


def test_torch_regulariser_and_step_against_statement():
    lo = cr.reg_layout()
    a = cr.reg_arena(2)
    x = torch.from_numpy(a).requires_grad_(True)
    reg = clarity.noise_reg_torch(x, lo)
    reg.sum().backward()
    reg64, g64 = cr.noise_reg_f64(a, lo).numpy(), cr.noise_reg_grad_f64(a, lo)
    assert np.abs(reg.detach().numpy() - reg64).max() <= 64 * cr.EPS32 * np.abs(reg64).max()
    assert np.abs(x.grad.numpy() - g64).max() <= 64 * cr.EPS32 * np.abs(g64).max()
    rs = np.random.RandomState(1)
    for t in (1, 2, 10):
        g = (rs.randn(2, lo.p) * 1e-3).astype(np.float32)
        g[:, lo.off[3]:lo.off[3] + lo.res[3] ** 2] = 0
        m = np.zeros_like(g) if t == 1 else (rs.randn(2, lo.p) * 1e-3).astype(np.float32)
        v = np.zeros_like(g) if t == 1 else ((np.abs(rs.randn(2, lo.p)) + 0.5) * 1e-6).astype(np.float32)
        ts = [torch.from_numpy(z.copy()) for z in (a, g, m, v)]
        clarity.step_torch(ts[0], ts[1], ts[2], ts[3], lo, 0.07, t)
        want = cr.step_f64(a, g, m, v, lo, 0.07, t)
        for got, w64, tol in zip((ts[0], ts[2], ts[3]), want, (2e-5, 1e-6, 1e-6)):
            assert np.abs(got.numpy() - w64).max() <= tol * max(1e-12, np.abs(w64).max()), t


def test_schedule_and_w_stats_against_golden(gold, tiny):
    cfg, sd = tiny
    n = int(gold["num_steps"])
    for s in range(n):
        lr, scale = clarity.lr_and_noise_schedule(s, n, float(gold["w_std"]))
        assert lr == gold["lr"][s] and scale == gold["w_noise_scale"][s]
        assert (lr, scale) == pytest.approx(cr.schedule_f64(s, n, float(gold["w_std"])), rel=1e-15, abs=0)
    assert clarity.lr_and_noise_schedule(0, 1000)[0] == 0.0 and clarity.lr_and_noise_schedule(50, 1000)[0] == pytest.approx(0.1)
    assert clarity.lr_and_noise_schedule(999, 1000, 2.0) == pytest.approx((0.1 * (0.5 - 0.5 * np.cos(0.004 * np.pi)), 0.0))
    w_avg, w_std = clarity.w_stats(cr.OracleGen(cfg, sd).mapping, cfg.z_dim, int(gold["w_stats_samples"]))
    assert w_avg.shape == gold["w_avg"].shape and np.abs(w_avg - gold["w_avg"]).max() <= 1e-6 and abs(w_std - float(gold["w_std"])) <= 1e-6 * w_std


# ------------------------------------------------------------------------------------------------
# the optimiser, route "torch", on the oracle
# ------------------------------------------------------------------------------------------------
def _optimizer(gold, tiny, draws, **kw):
    cfg, sd = tiny
    return clarity.ClarityOptimizer(cr.OracleGen(cfg, sd), cr.StandInEncoder(cfg), gold["drawings"], route="torch", w_std=float(gold["w_std"]),
                                    draws=draws, **kw)


def test_optimizer_reproduces_the_reference_run(gold, tiny):
    """Bound: eps_ref x FACTOR.  An error d in a gradient moves Adam's update lr * m_hat / (sqrt(v_hat) + eps) by at most
    2 lr d / sqrt(v_hat) (m_hat and sqrt(v_hat) each move by at most d, and |m_hat| <= sqrt(v_hat)); with d = eps_ref and the
    smallest sqrt(v_hat) of each step of this case (recorded from the float64 run: at t = 1 it is the smallest |g|) the steps add up
    to FACTOR = sum_t 2 lr_t / min sqrt(v_hat_t).  The renormalisation keeps the planes at unit scale.  The reference itself is
    within eps_ref (FACTOR >= 1) of the float64 run by the definition of eps_ref."""
    draws = cr.ReplayDraws(gold["init_noise"], gold["w_noise"], gold["drawing_idx"])
    opt = _optimizer(gold, tiny, draws)
    assert opt.fused and opt.item_names == ["iou_inv_uvs", "iou_u", "l1_fake_orig"] and opt.fused_weights == (0.5, 0.5, 50.0)
    rec = []
    out = opt.optimize(cr.DictLibrary(zs={"a": gold["z"]}), num_steps=int(gold["num_steps"]), batch_size=int(gold["batch"]),
                       on_step=lambda ids, s, lr, items, reg: rec.append((lr, items.numpy().copy(), reg.numpy().copy())))
    eps = float(gold["eps_ref"])
    factor = float(np.sum(2 * gold["lr"] / gold["adam_denom_min"]))
    assert factor >= 1
    lo = opt.layout
    row = np.concatenate([out["a"]["w"].numpy().reshape(-1)] + [out["a"]["noise"][n].numpy().reshape(-1) for n in lo.names])
    ref_row = np.concatenate([gold["final_w"].reshape(-1), gold["final_noise"]])
    items = np.array([r[1][0] for r in rec])[:, [opt.item_names.index(str(n)) for n in gold["item_names"]]]
    e_row, e_items = np.abs(row - ref_row).max(), np.abs(items - gold["items"]).max()
    e_reg = np.abs(np.array([r[2][0] for r in rec]) - gold["reg_ref_states"]).max()
    print(f"[clarity] torch route vs reference: final {e_row:.3g}, items {e_items:.3g}, reg {e_reg:.3g}; bound {eps * factor:.3g} (eps_ref {eps:.3g} x {factor:.3g})")
    assert e_row <= eps * factor and e_items <= eps * factor and e_reg <= eps * factor
    assert np.array_equal(np.array([r[0] for r in rec]), gold["lr"])
    assert np.abs(gold["final_row_f64"] - ref_row).max() <= eps * factor      # the reference alone stays inside the bound
    assert set(opt.history["a"]) == {"first", "last"} and opt.history["a"]["first"]["iou_inv_uvs"] == pytest.approx(gold["items"][0][_golden_order(gold, ["iou_inv_uvs"])[0]], abs=1e-5)


def test_two_brushes_equal_two_single_runs(gold, tiny):
    cfg, _ = tiny
    lib = cr.DictLibrary(zs={"a": gold["z"], "b": np.random.RandomState(9).randn(1, cfg.z_dim)})
    runs = {}
    for name, per_pass in (("together", 2), ("alone", 1)):
        opt = _optimizer(gold, tiny, None)
        runs[name] = opt.optimize(lib, num_steps=4, batch_size=3, brushes_per_pass=per_pass, seed=5)
    for sid in ("a", "b"):
        a, b = runs["together"][sid], runs["alone"][sid]
        assert float((a["w"] - b["w"]).abs().max()) <= 1e-5 * float(b["w"].abs().max())
        for n in a["noise"]:
            assert float((a["noise"][n] - b["noise"][n]).abs().max()) <= 1e-4, (sid, n)
    assert float((runs["alone"]["a"]["w"] - runs["alone"]["b"]["w"]).abs().max()) > 1e-2


def test_background_clears_on_held_out_drawings(gold, tiny):
    """'1.0*iou_inv(uvs)+1.0*iou(u)', 60 steps, batch 4: iou_inv(uvs) on drawings the run never saw ends below 0.6 of its start."""
    cfg, sd = tiny
    gen, enc = cr.OracleGen(cfg, sd), cr.StandInEncoder(cfg)
    opt = clarity.ClarityOptimizer(gen, enc, cr.line_drawings(32, 24, seed=0), losses="1.0*iou_inv(uvs)+1.0*iou(u)", route="torch", w_std=float(gold["w_std"]))
    assert not opt.fused and opt.item_names == ["iou_inv_uvs", "iou_u"]
    lib = cr.DictLibrary(zs={"a": gold["z"]})
    regs = []
    out = opt.optimize(lib, num_steps=60, batch_size=4, seed=0, on_step=lambda ids, s, lr, items, reg: regs.append(float(reg[0])))
    held = torch.from_numpy(cr.line_drawings(32, 8, seed=100)).float().div(255)[:, None]

    def iou_inv(w, noise):
        with torch.no_grad():
            _, raw = gen.synthesis(w.expand(len(held), -1, -1), enc(held), noise_buffers=noise, return_debug_data=True)
        return float(cr.loss_f64(raw["uvs"], raw["uvs"], raw["uvs"], held, 1, (1.0, 1.0, 0.0))[0][0, 0])

    start = {n: torch.from_numpy(np.asarray(sd["synthesis." + n])) for n in opt.layout.names}
    before, after = iou_inv(opt.start_w(lib, ["a"]), start), iou_inv(out["a"]["w"], out["a"]["noise"])
    print(f"[clarity] held-out iou_inv(uvs) {before:.3f} -> {after:.3f}; regulariser {regs[0]:.3g} -> {regs[-1]:.3g}")
    assert after < 0.6 * before and regs[-1] < 0.1 * regs[0]


def test_other_loss_strings_and_lpips(gold, tiny):
    cfg, sd = tiny
    mk = lambda s: clarity.ClarityOptimizer(cr.OracleGen(cfg, sd), cr.StandInEncoder(cfg), gold["drawings"], losses=s, route="torch", w_std=1.0)
    with pytest.raises(RuntimeError, match="LPIPS"):
        mk("0.5*iou_inv(uvs)+0.5*iou(u)+50*lpips(fake_orig)+50*l1(fake_orig)")
    assert mk("2*l1(fake_orig)+iou(u)+0.1*iou_inv(uvs)").fused_weights == (0.1, 1.0, 2.0)
    assert not mk("0.5*iou_inv(uvs)+0.5*dice(uvs)").fused
    with pytest.raises(_lib.NeubeHipError):
        clarity.ClarityOptimizer(cr.OracleGen(cfg, sd), cr.StandInEncoder(cfg), gold["drawings"], route="hip", w_std=1.0)
    with pytest.raises(ValueError):
        clarity.ClarityOptimizer(cr.OracleGen(cfg, sd), cr.StandInEncoder(cfg), gold["drawings"][:, :16], route="torch")
    # the generic path and the fused arithmetic agree on the three default items
    opt_f, opt_g = mk(clarity.DEFAULT_LOSSES), mk(clarity.DEFAULT_LOSSES)
    opt_g.fused = False
    opt_g.item_names = [l.full_name() for l in opt_g.losses.losses]
    lo = opt_f.layout
    rs = np.random.RandomState(2)
    arena = torch.from_numpy(rs.randn(2, lo.p).astype(np.float32))
    geom = torch.from_numpy(gold["drawings"][:3].astype(np.float32) / 255)[:, None]
    args = (arena, lo.w(arena).clone(), torch.from_numpy(0.05 * rs.randn(2, *lo.w_shape).astype(np.float32)), geom)
    (g1, i1, r1), (g2, i2, r2) = opt_f.loss_and_grad(*args), opt_g.loss_and_grad(*args)
    assert float((g1 - g2).abs().max()) <= 1e-4 * float(g2.abs().max()) and float((i1 - i2).abs().max()) <= 1e-6 and torch.equal(r1, r2)


# ------------------------------------------------------------------------------------------------
# formats, command line
# ------------------------------------------------------------------------------------------------
def _fake_result(cfg, ids, seed=0):
    lo, rs = clarity.ArenaLayout.from_config(cfg), np.random.RandomState(seed)
    return {i: {"w": torch.from_numpy(rs.randn(1, cfg.num_ws, cfg.w_dim).astype(np.float32)),
                "noise": {n: torch.from_numpy(rs.randn(r, r).astype(np.float32)) for n, r in zip(lo.names, lo.res)}} for i in ids}


def test_result_round_trips_through_the_w_library(tiny, tmp_path):
    cfg, _ = tiny
    res = _fake_result(cfg, ["7", "9"])
    path = str(tmp_path / "lib.pkl")
    brush_clarity_main.merge_into_library(path, res)
    lib = formats.BrushLibrary.from_file(path)
    assert isinstance(lib, formats.WBrushLibrary) and lib.get_style_ids() == ["7", "9"]
    opts = painting.GanBrushOptions()
    lib.set_style("9", opts)
    assert torch.equal(opts.style_ws, res["9"]["w"]) and opts.style_z is None
    bufs = opts.custom_args["noise_buffers"]
    assert sorted(bufs) == sorted(res["9"]["noise"]) and all(torch.equal(bufs[k], v) for k, v in res["9"]["noise"].items())


def test_cli_parser_merge_and_records(tiny, tmp_path, caplog):
    cfg, _ = tiny
    ap = brush_clarity_main.build_parser()
    a = ap.parse_args(["--gan_checkpoint", "e.npz", "--library", "rand4", "--drawings", "d.npz", "--out_library", "default", "--output_dir", "o"])
    assert (a.batch_size, a.num_steps, a.brushes_per_pass, a.seed, a.brush_id, a.uvs_calibration) == (20, 1000, 4, None, None, None)
    assert a.losses == clarity.DEFAULT_LOSSES == "0.5*iou_inv(uvs)+0.5*iou(u)+50*l1(fake_orig)"
    a = ap.parse_args(["--gan_checkpoint", "e.npz", "--library", "l.pkl", "--drawings", "d.npz", "--out_library", "x.pkl", "--output_dir", "o", "--brush_id",
                       "12", "--batch_size", "8", "--num_steps", "30", "--losses", "1.0*iou_inv(uvs)", "--seed", "3", "--brushes_per_pass", "2",
                       "--uvs_calibration", "c.npz"])
    assert (a.brush_id, a.batch_size, a.num_steps, a.losses, a.seed, a.brushes_per_pass, a.uvs_calibration) == ("12", 8, 30, "1.0*iou_inv(uvs)", 3, 2, "c.npz")
    with pytest.raises(SystemExit):
        ap.parse_args(["--library", "rand4"])
    libfile = tmp_path / "sub" / "brushes.txt"
    libfile.parent.mkdir()
    libfile.write_text("1\n2\n")
    assert brush_clarity_main.default_out_library(str(libfile), "o") == str(tmp_path / "sub" / "OPT_brushes.txt")
    assert brush_clarity_main.default_out_library("rand4", "o") == os.path.join("o", "OPT_rand4.pkl")
    # merge: a second write keeps what is there, overwrites with a warning
    path = str(tmp_path / "out" / "lib.pkl")
    first, second = _fake_result(cfg, ["1", "2"], 0), _fake_result(cfg, ["2", "3"], 1)
    brush_clarity_main.merge_into_library(path, first)
    with caplog.at_level("WARNING"):
        brush_clarity_main.merge_into_library(path, second)
    assert any("already has projection for 2" in r.message for r in caplog.records) and not any("for 3" in r.message for r in caplog.records)
    with open(path, "rb") as f:
        data = pickle.load(f)
    assert sorted(data) == ["1", "2", "3"] and torch.equal(data["1"]["w"], first["1"]["w"]) and torch.equal(data["2"]["w"], second["2"]["w"])
    # records
    from brushstroke_engine_amd.metrics import BrushScores
    sc = lambda x: BrushScores(["2", "3"], lab_e_percent=np.zeros(2, np.float32), lab_l2=np.zeros(2, np.float32),
                               bg_clarity_mean=np.array([x, x + 0.1], np.float32), fg_opacity_median=np.array([0.9, 0.8], np.float32))
    hist = {"2": {"first": {"iou_inv_uvs": 0.7, "noise_reg": 0.2}, "last": {"iou_inv_uvs": 0.2, "noise_reg": 0.001}}}
    info = brush_clarity_main.write_records(str(tmp_path / "rec"), second, hist, sc(0.5), sc(0.8))
    with open(info) as f:
        j = json.load(f)
    assert os.path.basename(info) == "clarity.json" and sorted(j) == ["2", "3"]
    assert j["2"]["first"]["iou_inv_uvs"] == 0.7 and j["2"]["before"]["BG_CLARITY_MEAN"] == pytest.approx(0.5) and j["3"]["after"]["BG_CLARITY_MEAN"] == pytest.approx(0.9)
    with np.load(str(tmp_path / "rec" / "3_opt_optimized.npz")) as z:
        assert np.array_equal(z["w"], second["3"]["w"].numpy()) and "b4.conv1.noise_const" in z.files


# ------------------------------------------------------------------------------------------------
# the C entries: host-side argument checks, header, build
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def library():
    build.build()
    return _lib.lib()


def _planes(res, nw):
    return clarity.ArenaLayout(nw, res).planes_struct()


def test_entry_argument_checks(library):
    err = lambda: library.nb_last_error().decode()
    P = 0x1000                                                             # never dereferenced: the checks come before any HIP call
    # loss
    assert library.nb_clarity_loss_f32(None, 192, P, 192, P, 192, P, 1, 1, 8, 0.5, 0.5, 50.0, P, P, P, None) == _lib.NB_EINVAL and "null pointer" in err()
    assert library.nb_clarity_loss_f32(P, 192, P, 192, P, 192, P, 1, 0, 8, 0.5, 0.5, 50.0, P, P, P, None) == _lib.NB_EINVAL and "bad sizes" in err()
    assert library.nb_clarity_loss_f32(P, 192, P, 192, P, 192, P, 4096, 16, 8, 0.5, 0.5, 50.0, P, P, P, None) == _lib.NB_EINVAL and "k * b <= 65535" in err()
    assert library.nb_clarity_loss_f32(P, 191, P, 192, P, 192, P, 1, 1, 8, 0.5, 0.5, 50.0, P, P, P, None) == _lib.NB_EINVAL and "stride" in err()
    assert library.nb_clarity_loss_f32(P + 2, 192, P, 192, P, 192, P, 1, 1, 8, 0.5, 0.5, 50.0, P, P, P, None) == _lib.NB_EINVAL and "aligned" in err()
    assert library.nb_clarity_loss_f32(P, 192, P, 192, P, 192, P, 0, 1, 8, 0.5, 0.5, 50.0, P, P, P, None) == _lib.NB_OK
    assert library.nb_clarity_loss_bwd_f32(P, 192, P, 192, P, None, None, 1, 1, 8, 0.5, 0.5, 50.0, P, P, None) == _lib.NB_EINVAL and "null pointer" in err()
    assert library.nb_clarity_loss_bwd_f32(P, 192, P, 10, P, P, None, 1, 1, 8, 0.5, 0.5, 50.0, P, P, None) == _lib.NB_EINVAL and "stride" in err()
    assert library.nb_clarity_loss_bwd_f32(P, 192, P, 192, P, P, P + 1, 1, 1, 8, 0.5, 0.5, 50.0, P, P, None) == _lib.NB_EINVAL and "aligned" in err()
    assert library.nb_clarity_loss_bwd_f32(P, 192, P, 192, P, P, None, 0, 1, 8, 0.5, 0.5, 50.0, P, P, None) == _lib.NB_OK
    # layouts
    good = _planes([4, 8, 16], 40)
    p = 40 + 16 + 64 + 256
    need = library.nb_clarity_scratch_floats(C.byref(good), 40, p, 2)
    assert need == 2 * max(16 * 3 + 64, 2 * (1 + 1 + 1 + 1))
    reg = lambda pl, nw=40, p_=p, k=1, scratch=10 ** 6, arena=P, stride=None: library.nb_noise_reg_f32(
        arena, p_ if stride is None else stride, p_, nw, C.byref(pl) if pl is not None else None, k, 10.0, P, p_, P, P, scratch, None)
    assert reg(None) == _lib.NB_EINVAL and "null pointer" in err()
    assert reg(good, arena=None) == _lib.NB_EINVAL and "null pointer" in err()
    bad = _planes([4, 8, 16], 40)
    bad.res[1] = 12
    assert reg(bad) == _lib.NB_EINVAL and "power of two" in err()
    bad.res[1] = 512
    assert reg(bad) == _lib.NB_EINVAL and "power of two" in err()
    bad = _planes([4, 8, 16], 40)
    bad.off[2] -= 1
    assert reg(bad) == _lib.NB_EINVAL and "overlaps" in err()
    bad = _planes([4, 8, 16], 40)
    bad.off[0] = 39
    assert reg(bad) == _lib.NB_EINVAL and "overlaps" in err()
    assert reg(good, p_=p - 1) == _lib.NB_EINVAL and "leaves the row" in err()
    bad = _planes([4], 0)
    bad.n = 33
    assert reg(bad) == _lib.NB_EINVAL and "plane count" in err()
    assert reg(good, k=-1) == _lib.NB_EINVAL and "outside 0..65535" in err()
    assert reg(good, stride=p - 1) == _lib.NB_EINVAL and "row stride" in err()
    assert reg(good, k=2, scratch=need - 1) == _lib.NB_EINVAL and "too small" in err() and str(2 * (16 * 3 + 64)) in err()
    assert reg(good, k=0) == _lib.NB_OK
    assert library.nb_clarity_scratch_floats(C.byref(bad), 0, 16, 1) == -1 and "plane count" in err()
    # step
    step = lambda pl=good, k=1, t=1, scratch=10 ** 6, grad=P, stride=p: library.nb_clarity_step_f32(P, grad, P, P, stride, p, 40, C.byref(pl), k, 0.1, t, P, scratch,
                                                                                                  None)
    assert step(grad=None) == _lib.NB_EINVAL and "null pointer" in err()
    assert step(t=0) == _lib.NB_EINVAL and "below 1" in err()
    assert step(stride=p - 1) == _lib.NB_EINVAL and "row stride" in err()
    assert step(grad=P + 2) == _lib.NB_EINVAL and "aligned" in err()
    assert step(k=3, scratch=3 * 8 - 1) == _lib.NB_EINVAL and "too small" in err()
    assert step(k=0) == _lib.NB_OK


def test_header_abi_version_and_sources(library):
    text = open(os.path.join(REPO, "include", "neube_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
        assert name in _lib.PROTOTYPES and hasattr(library, name)
    assert "opt_clarity_main.py:127-137" in text and "opt_clarity_main.py:163-167" in text and "forger/train/losses.py" in text
    assert re.search(r"#define NB_ABI_VERSION 22\b", open(os.path.join(build.CSRC, "nb_common.h")).read())
    assert _lib.ABI_VERSION == 22 and library.nb_abi_version() == 22
    assert "nb_clarity.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "nb_clarity.hip"))
    assert C.sizeof(_lib.NbClarityPlanes) == 4 * (1 + 2 * _lib.NB_CLARITY_MAX_PLANES)
    for k, v in (("NB_CLARITY_MAX_PLANES", _lib.NB_CLARITY_MAX_PLANES), ("NB_CLARITY_LOSS_PARTS", _lib.NB_CLARITY_LOSS_PARTS), ("NB_CLARITY_CHUNK", _lib.NB_CLARITY_CHUNK)):
        assert re.search(rf"#define {k} {v}\b", text), k
