"""Child process of tests/test_hip_capi.py: one group of checks of the C generator entry (nb_generator_*) on the GPU.

    python tests/_capi_worker.py packers                # device packers == torch packers (style1, tests/_gen_configs.py, ragged shapes)
    python tests/_capi_worker.py python <mode> <R>      # NativeGenerator == Generator.render_triad, describe == layer_kernels, errors
    python tests/_capi_worker.py matrix <config> <mode> # the same at every batch threshold for a tests/_gen_configs.py net + its rows
    python tests/_capi_worker.py oracle <config>        # the C entry against the float64 oracle, all modes
    python tests/_capi_worker.py golden <mode>          # the C entry against the reference's golden vectors
    python tests/_capi_worker.py graph <mode> <R>       # captured C forward == eager C forward
    python tests/_capi_worker.py chost <exe> <workdir>  # examples/capi/generate.c == NativeGenerator

Prints one line per check and exits non-zero at the first failure (the parent shows the output)."""
import os
import subprocess
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from brushstroke_engine_amd import _lib, config as cfgmod, ops, synthetic, weights as wmod  # noqa: E402
from brushstroke_engine_amd.native import NativeGenerator, pack_weights_dev  # noqa: E402
from brushstroke_engine_amd.networks import Generator  # noqa: E402

DEV = torch.device("cuda:0")
PIX = {"f32": 1e-4, "h3": 1e-4, "f8": 3e-4}
BATCHES = (1, 5, 16, 32)


def D(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def check(ok, what):
    print(("ok   " if ok else "FAIL ") + what, flush=True)
    if not ok:
        sys.exit(1)


def ulps(a, b):
    ia = a.view(torch.int32).to(torch.int64)
    ib = b.view(torch.int32).to(torch.int64)
    return int((ia - ib).abs().max()) if a.numel() else 0


def inputs(cfg, n, seed):
    return (D(synthetic.batch_z(cfg, n, seed).astype(np.float32)), [D(g) for g in synthetic.geom_features(cfg, n, seed=seed)],
            D(synthetic.positions(cfg, n, seed=seed)))


# (c_out, c_in) beside the nets' own layers: single channels, c_in not a multiple of 8 or 16, partial 64-channel c_out slices
PACK_SHAPES = ((1, 1), (3, 5), (21, 105), (100, 121), (72, 112), (160, 416), (64, 40))


def check_packers(w, what, f=None):
    """Every device packer == its torch packer for one weight; h3_up2 only when f is given.  Returns the wsq ulp difference."""
    wpk, wsq = ops.pack_conv_weight(w)
    dpk, dsq = pack_weights_dev(w, "wpk")
    check(torch.equal(wpk, dpk), f"{what} wpk")
    check(torch.equal(ops.pack_conv_weight_h3(w).view(torch.int16), pack_weights_dev(w, "h3").view(torch.int16)), f"{what} w_h3")
    check(torch.equal(ops.pack_conv_weight_h3f8(w).view(torch.int16), pack_weights_dev(w, "f8").view(torch.int16)), f"{what} w_f8")
    if f is not None:
        want = ops.pack_conv_weight_h3_up2_phases(w, f)
        check(torch.equal(want.view(torch.int16), pack_weights_dev(w, "h3_up2", f).view(torch.int16)), f"{what} w_h3_up2")
    return ulps(wsq, dsq)


def packers():
    from _gen_configs import CONFIGS
    nets = [(f"R={res}", cfgmod.style1_config(res), True) for res in (128, 256)]
    nets += [(cid, cfg, False) for cid, (cfg, _) in CONFIGS.items()]
    filt = None
    for label, cfg, every_up2 in nets:
        sd = wmod.random_state_dict(cfg, seed=3)
        worst_wsq = 0
        for s in cfg.layers:
            f = D(sd[f"{s.name}.resample_filter"])
            filt = f
            # the phase kernels as nb_generator_create packs them (up=2, input <= 32x32, whole 16-channel chunks); style1: every up=2 layer
            up2 = s.up == 2 and (every_up2 or (s.in_res <= 32 and s.in_channels % 16 == 0))
            worst_wsq = max(worst_wsq, check_packers(D(sd[f"{s.name}.weight"]), f"{label} {s.name}", f if up2 else None))
        print(f"[capi] {label} wsq max ulp difference to torch: {worst_wsq}", flush=True)
        check(worst_wsq == 0, f"{label} wsq bitwise")
    rs = np.random.RandomState(17)
    worst_wsq = 0
    for co, ci in PACK_SHAPES:
        w = D((rs.randn(co, ci, 3, 3) * rs.choice([1e-3, 1.0, 30.0], size=(co, ci, 1, 1))).astype(np.float32))
        worst_wsq = max(worst_wsq, check_packers(w, f"[{co}, {ci}, 3, 3]", filt if ci % 16 == 0 else None))
    print(f"[capi] ragged shapes wsq max ulp difference to torch: {worst_wsq}", flush=True)
    check(worst_wsq == 0, "ragged shapes wsq bitwise")


def python_pass(G, geom, kw, nkw):
    """Generator.render_triad as one chain -> ((u8, rgba, uvs, colors, img), layer_kernels, layer_formats); img comes from a second
    pass over the same inputs (render_triad does not return it)."""
    u8, rgba, dbg = G.render_triad(geom_feature=geom, want_f32=True, **kw, **nkw)
    kernels, formats = dict(G.synthesis.layer_kernels), dict(G.synthesis.layer_formats)
    xkw = {k: v for k, v in kw.items() if k not in ("z", "ws")}
    extra = {"rgba_u8": False, "rgba": False, "render_mode": xkw.pop("render_mode", "clear"), "user_colors": xkw.pop("user_colors", None),
             "sfactor": xkw.pop("sfactor", None)}
    if "z" in kw:
        img, _ = G(kw["z"], None, geom, return_debug_data=True, _extra_outputs=extra, noise_mode=nkw.get("noise_mode", "const"), **xkw)
    else:
        img, _ = G.forward_pre_mapped(kw["ws"], geom, return_debug_data=True, _extra_outputs=extra,
                                      noise_mode=nkw.get("noise_mode", "const"), **xkw)
    return (u8, rgba, dbg["uvs"], dbg["colors"], img), kernels, formats


def c_pass(ng, geom, kw, nkw):
    cu8, crgba, cdbg = ng.render_triad(geom_feature=geom, want_f32=True, **kw, **nkw)
    return cu8, crgba, cdbg["uvs"], cdbg["colors"], cdbg["img"]


def check_bitwise(py, c, what):
    eq = lambda a, b: a is None and b is None or (a is not None and b is not None and torch.equal(a, b))   # noqa: E731
    torch.cuda.synchronize()
    same = all(eq(a, b) for a, b in zip(py, c))
    if not same:
        (u8, rgba, uvs, colors, img), (cu8, crgba, cuvs, ccolors, cimg) = py, c
        print(f"  u8 {int((u8.int() - cu8.int()).abs().max())} rgba {float((rgba - crgba).abs().max()):.3e} "
              f"uvs {float((uvs - cuvs).abs().max()):.3e} colors {float((colors - ccolors).abs().max()):.3e} "
              f"img {float((img - cimg).abs().max()):.3e}", flush=True)
    check(same, f"{what}: bitwise equal to Generator.render_triad")


def python_vs_c(mode, res):
    cfg = cfgmod.style1_config(res)
    sd = wmod.random_state_dict(cfg, seed=5)
    G = Generator(cfg, sd, conv_mode=mode).to(DEV)
    G.sub_stream_min_batch = 10 ** 9                         # the Python pass as one chain too
    ng = NativeGenerator.from_generator(G, n_max=max(BATCHES))
    for n in BATCHES:
        z, geom, pos = inputs(cfg, n, 100 + n)
        rs = np.random.RandomState(n)
        user = rs.rand(n, 3, 3).astype(np.float32)
        user[rs.rand(n, 3, 3) < 0.3] = np.nan                  # NaN = the style's own colour
        sfac = D((0.5 + rs.rand(n)).astype(np.float32))
        ws = G.mapping(z, None)
        cases = [("z+positions", dict(z=z, positions=pos), {}),
                 ("no positions", dict(z=z), {}),
                 ("noise none", dict(z=z, positions=pos), dict(noise_mode="none")),
                 ("full+user+sfactor", dict(z=z, positions=pos, render_mode="full", user_colors=D(user), sfactor=sfac), {}),
                 ("scalar sfactor", dict(z=z, positions=pos, sfactor=0.8), {}),
                 ("ws input", dict(ws=ws, positions=pos), {})]
        for name, kw, nkw in cases:
            py, kernels, _ = python_pass(G, geom, kw, nkw)
            check_bitwise(py, c_pass(ng, geom, kw, nkw), f"{mode} R={res} n={n} {name}")
        desc = ng.describe(n)
        check(desc == kernels, f"{mode} R={res} n={n} describe == layer_kernels")
        # truncation: torch's lerp bits are not guaranteed -> within the mode's pixel tolerance
        u8, rgba, dbg = G.render_triad(z=z, geom_feature=geom, positions=pos, want_f32=True, truncation_psi=0.7, truncation_cutoff=8)
        cu8, crgba, cdbg = ng.render_triad(z=z, geom_feature=geom, positions=pos, want_f32=True, truncation_psi=0.7, truncation_cutoff=8)
        e = max(float((rgba - crgba).abs().max()), float((dbg["uvs"] - cdbg["uvs"]).abs().max()))
        check(e <= PIX[mode] and int((u8.int() - cu8.int()).abs().max()) <= 1, f"{mode} R={res} n={n} truncation 0.7: {e:.2e}")
    # errors: nothing is enqueued
    lib = _lib.lib()
    n = 4
    z, geom, pos = inputs(cfg, n, 7)
    outs = {"uvs": torch.full([ng.n_max + 1, 3, res, res], 7.0, device=DEV)}
    for what, kw, nn, code in (("n > n_max", dict(z=torch.zeros(ng.n_max + 1, cfg.z_dim, device=DEV), geom_feature=[g.repeat(9, 1, 1, 1)[:ng.n_max + 1] for g in geom]),
                                ng.n_max + 1, _lib.NB_EINVAL),
                               ("NULL z and ws", dict(geom_feature=geom), n, _lib.NB_EINVAL),
                               ("NULL geometry", dict(z=z, geom_feature=[geom[0], None]), n, _lib.NB_EINVAL),
                               ("random noise", dict(z=z, geom_feature=geom, noise_mode="random"), n, _lib.NB_EUNSUPPORTED)):
        try:
            ng.forward_into(outs, nn, **kw)
            rc = 0
        except _lib.NeubeHipError as e:
            rc = int(str(e).split("(")[1].split(")")[0])
        torch.cuda.synchronize()
        check(rc == code and bool((outs["uvs"] == 7.0).all()), f"error {what}: code {rc}, nothing written ({lib.nb_last_error().decode()})")
    ng.close()


def matrix(cid, mode):
    """A tests/_gen_configs.py net through the C entry and the Python pass at every batch of BATCHES: the kernel plan first (nothing
    is enqueued through the C entry before its plan matches), then bitwise equality, then the decision rows the net exists for."""
    from _gen_configs import BATCHES as NS, CONFIGS, expected_rows, rows_reached
    cfg = CONFIGS[cid][0]
    G = Generator(cfg, wmod.random_state_dict(cfg, seed=5), conv_mode=mode).to(DEV)
    G.sub_stream_min_batch = 10 ** 9
    ng = NativeGenerator.from_generator(G, n_max=max(NS))
    reached = set()
    for n in NS:
        z, geom, pos = inputs(cfg, n, 200 + n)
        ws = G.mapping(z, None)
        for k, (name, kw) in enumerate((("z+positions", dict(z=z, positions=pos)), ("ws input", dict(ws=ws, positions=pos)))):
            py, kernels, formats = python_pass(G, geom, kw, {})
            if k == 0:
                desc = ng.describe(n)
                if desc != kernels:
                    for key in sorted(set(desc) | set(kernels)):
                        if desc.get(key) != kernels.get(key):
                            print(f"  {key}: C {desc.get(key)}, Python {kernels.get(key)}", flush=True)
                check(desc == kernels, f"{cid} {mode} n={n} describe == layer_kernels")
                rows = rows_reached(cfg, mode, kernels, formats)
                reached |= rows
                print(f"[capi rows] {cid} {mode} n={n}: {' '.join(sorted(rows)) or '-'}", flush=True)
            check_bitwise(py, c_pass(ng, geom, kw, {}), f"{cid} {mode} n={n} {name}")
    missing = expected_rows(cid, mode) - reached
    check(not missing, f"{cid} {mode} reaches its rows {sorted(expected_rows(cid, mode))} (missing: {sorted(missing)})")
    ng.close()


def oracle_batch(cfg, sd, n=32):
    """One float64 CPU oracle pass on a batch of n (constant noise, positions): (z, geom, positions, oracle debug dict)."""
    from oracle import neube_oracle as orc
    z, geom, pos = synthetic.batch_z(cfg, n, 300), synthetic.geom_features(cfg, n, seed=30), synthetic.positions(cfg, n, seed=30)
    img, want = orc.OracleGenerator(cfg, sd, dtype=torch.float64)(z, None, geom, positions=pos, return_debug_data=True,
                                                                  return_features=[cfg.img_resolution // 2])
    want["img"] = img
    return z, geom, pos, want


def oracle(cid):
    """The C entry of a tests/_gen_configs.py net against the float64 oracle, in every mode, at n = 32 and on the first 1 / 9 / 16
    samples of the same batch."""
    from _gen_configs import CONFIGS
    cfg = CONFIGS[cid][0]
    sd = wmod.random_state_dict(cfg, seed=6)
    z, geom, pos, want = oracle_batch(cfg, sd)
    for mode in ("f32", "h3", "f8"):
        ng = NativeGenerator.from_state_dict(cfg, sd, mode, 32, DEV)
        worst = {"uvs": 0.0, "img": 0.0, "colors": 0.0}
        for n in (32, 1, 9, 16):
            _, _, dbg = ng.render_triad(z=D(z[:n]), geom_feature=[D(g[:n]) for g in geom], positions=D(pos[:n]))
            e = {k: float((dbg[k].cpu().double() - want[k][:n]).abs().max()) for k in worst}
            worst = {k: max(worst[k], e[k]) for k in worst}
            check(e["uvs"] <= PIX[mode] and e["img"] <= PIX[mode] and e["colors"] <= 1e-5,
                  f"{cid} {mode} n={n} vs float64 oracle: uvs {e['uvs']:.2e} img {e['img']:.2e} colors {e['colors']:.2e}")
        print(f"[capi oracle] {cid} {mode} max error: " + " ".join(f"{k} {v:.2e}" for k, v in worst.items()), flush=True)
        ng.close()


def golden(mode):
    sys.path.insert(0, os.path.join(REPO, "tests"))
    from conftest import load_golden
    for res in (128, 256):
        g = load_golden(f"gen_r{res}.npz")
        cfg = cfgmod.style1_config(res)
        ng = NativeGenerator.from_state_dict(cfg, wmod.random_state_dict(cfg, seed=int(g["weights_seed"])), mode, 2, DEV)
        geom = [D(x) for x in synthetic.geom_features(cfg, 2, seed=int(g["geom_seed"]))]
        _, _, dbg = ng.render_triad(z=D(g["z"]), geom_feature=geom, positions=D(g["positions"]))
        s = int(g["step"])
        e_c = float(np.abs(dbg["colors"].cpu().numpy() - g["colors"]).max())
        e_u = float(np.abs(dbg["uvs"].cpu().numpy()[..., ::s, ::s] - g["uvs.sub"]).max())
        e_i = float(np.abs(dbg["img"].cpu().numpy()[..., ::s, ::s] - g["img.sub"]).max())
        e_r = float(np.abs(dbg["uvs"].cpu().numpy()[:, :, res // 3, :] - g["uvs.row"]).max())
        print(f"[capi golden R={res} {mode}] colors {e_c:.2e} uvs {e_u:.2e} img {e_i:.2e} uvs.row {e_r:.2e}", flush=True)
        check(e_c <= 1e-5 and max(e_u, e_i, e_r) <= PIX[mode], f"gen_r{res} {mode}")
        ng.close()
    # tiny net (R=32, the small-image kernels): the cases of gen_tiny.npz whose inputs the C entry takes (A: z + positions, B: no positions)
    g = load_golden("gen_tiny.npz")
    cfg = cfgmod.tiny_config(32)
    ng = NativeGenerator.from_state_dict(cfg, wmod.random_state_dict(cfg, seed=int(g["weights_seed"])), mode, 3, DEV)
    geom = [D(x) for x in synthetic.geom_features(cfg, 3, seed=int(g["geom_seed"]))]
    _, _, a = ng.render_triad(z=D(g["z"]), geom_feature=geom, positions=D(g["positions"]))
    _, _, b = ng.render_triad(z=D(g["z"]), geom_feature=geom)
    e = {"A colors": float(np.abs(a["colors"].cpu().numpy() - g["A_colors"]).max()),
         "A uvs": float(np.abs(a["uvs"].cpu().numpy() - g["A_uvs"]).max()), "A img": float(np.abs(a["img"].cpu().numpy() - g["A_img"]).max()),
         "B img": float(np.abs(b["img"].cpu().numpy() - g["B_img"]).max())}
    print(f"[capi golden tiny {mode}] " + " ".join(f"{k} {v:.2e}" for k, v in e.items()), flush=True)
    check(e["A colors"] <= 1e-5 and max(e["A uvs"], e["A img"], e["B img"]) <= PIX[mode], f"gen_tiny {mode}")
    ng.close()
    # ten layers at the conv_clamp (the bounds of test_hip_generator.py::test_high_dynamic_range_fixture)
    g = load_golden("gen_hdr_r128.npz")
    cfg = cfgmod.style1_config(128)
    ng = NativeGenerator.from_state_dict(cfg, wmod.hdr_state_dict(cfg, seed=int(g["weights_seed"])), mode, 2, DEV)
    geom = [D(x) for x in synthetic.geom_features(cfg, 2, seed=int(g["geom_seed"]))]
    _, _, dbg = ng.render_triad(z=D(g["z"]), geom_feature=geom, positions=D(g["positions"]))
    e = {k: float(np.abs(dbg[k].cpu().numpy() - g[k]).max()) for k in ("colors", "uvs", "img")}
    print(f"[capi golden hdr {mode}] " + " ".join(f"{k} {v:.2e}" for k, v in e.items()), flush=True)
    check(e["colors"] <= 1e-5 and e["uvs"] <= 1e-3 and e["img"] <= 1e-3, f"gen_hdr_r128 {mode}")
    ng.close()
    # trained-like weight statistics (the colors / uvs / img bounds of test_hip_generator.py::test_trained_like_fixture)
    g = load_golden("gen_trained_r128.npz")
    ng = NativeGenerator.from_state_dict(cfg, wmod.trained_like_state_dict(cfg, seed=int(g["weights_seed"])), mode, 6, DEV)
    geom = [D(x) for x in synthetic.geom_features(cfg, 6, seed=int(g["geom_seed"]))]
    _, _, dbg = ng.render_triad(z=D(g["z"]), geom_feature=geom, positions=D(g["positions"]))
    e = {"colors": float(np.abs(dbg["colors"].cpu().numpy() - g["colors"]).max()),
         "uvs": float(np.abs(dbg["uvs"].cpu().numpy() - g["uvs"]).max()),
         "img.sub": float(np.abs(dbg["img"].cpu().numpy()[..., ::2, ::2] - g["img.sub"]).max())}
    print(f"[capi golden trained {mode}] " + " ".join(f"{k} {v:.2e}" for k, v in e.items()), flush=True)
    check(e["colors"] <= 1e-5 and e["uvs"] <= PIX[mode] and e["img.sub"] <= PIX[mode], f"gen_trained_r128 {mode}")
    ng.close()
    g = load_golden("gen_b32_r256.npz")
    cfg = cfgmod.style1_config(256)
    n = 32
    ng = NativeGenerator.from_state_dict(cfg, wmod.random_state_dict(cfg, seed=int(g["weights_seed"])), mode, n, DEV)
    z = D(synthetic.batch_z(cfg, n, int(g["first_seed"])))
    geom = [D(x) for x in synthetic.geom_features(cfg, n, seed=int(g["geom_seed"]))]
    pos = D(synthetic.positions(cfg, n, seed=int(g["pos_seed"])))
    _, _, dbg = ng.render_triad(z=z, geom_feature=geom, positions=pos)
    tol = PIX[mode]
    uvs, img = dbg["uvs"], dbg["img"]
    e = {"colors": float(np.abs(dbg["colors"].cpu().numpy() - g["colors"]).max()),
         "uvs.row": float(np.abs(uvs[:, :, 85, :].cpu().numpy() - g["uvs.row"]).max()),
         "img.row": float(np.abs(img[:, :, 170, :].cpu().numpy() - g["img.row"]).max()),
         "uvs.sub": float(np.abs(uvs[:, :, ::32, ::32].cpu().numpy() - g["uvs.sub"]).max())}
    print(f"[capi golden b32 R=256 {mode}] " + " ".join(f"{k} {v:.2e}" for k, v in e.items()), flush=True)
    check(e["colors"] <= 1e-5 and max(e["uvs.row"], e["img.row"], e["uvs.sub"]) <= tol, f"gen_b32_r256 {mode}")
    for name, t in (("uvs", uvs), ("img", img)):
        t64 = t.double()
        s1, s2 = t64.sum(dim=(2, 3)).cpu().numpy(), (t64 * t64).sum(dim=(2, 3)).cpu().numpy()
        check(np.abs(s1 - g[f"{name}.sum"]).max() <= 65536 * tol * 0.05 and np.abs(s2 - g[f"{name}.sumsq"]).max() <= 65536 * tol * 0.1,
              f"gen_b32_r256 {mode} {name} checksums")
    ng.close()


def graph(mode, res):
    cfg = cfgmod.style1_config(res)
    sd = wmod.random_state_dict(cfg, seed=9)
    for n in (1, 32):
        ng = NativeGenerator.from_state_dict(cfg, sd, mode, n, DEV)
        z, geom, pos = inputs(cfg, n, 11)
        r = res
        outs = {"rgba_u8": torch.empty([n, r, r, 4], dtype=torch.uint8, device=DEV), "rgba": torch.empty([n, 4, r, r], device=DEV),
                "uvs": torch.empty([n, 3, r, r], device=DEV), "img": torch.empty([n, 3, r, r], device=DEV),
                "colors": torch.empty([n, 3, 3], device=DEV)}
        ng.forward_into(outs, n, z=z, geom_feature=geom, positions=pos)          # eager: sets the kernels' attributes
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            ng.forward_into(outs, n, z=z, geom_feature=geom, positions=pos)
        z2, geom2, pos2 = inputs(cfg, n, 12)
        z.copy_(z2)
        pos.copy_(pos2)
        for a, b in zip(geom, geom2):
            a.copy_(b)
        for t in outs.values():
            t.zero_()
        gr.replay()
        want = {k: torch.empty_like(v) for k, v in outs.items()}
        ng.forward_into(want, n, z=z2, geom_feature=geom2, positions=pos2)
        torch.cuda.synchronize()
        check(all(torch.equal(outs[k], want[k]) for k in outs), f"{mode} R={res} n={n}: graph replay on new inputs == eager")
        del gr
        ng.close()


def chost(exe, work):
    cfg = cfgmod.style1_config(128)
    n, mode = 4, "f8"
    sd = wmod.random_state_dict(cfg, seed=13)
    from brushstroke_engine_amd.native import param_table
    with open(os.path.join(work, "weights.bin"), "wb") as f:
        for name, _ in param_table(cfg):
            f.write(np.ascontiguousarray(np.asarray(sd[name], np.float32)).tobytes())
    z = synthetic.batch_z(cfg, n, 21).astype(np.float32)
    geom = synthetic.geom_features(cfg, n, seed=21)
    pos = synthetic.positions(cfg, n, seed=21)
    with open(os.path.join(work, "inputs.bin"), "wb") as f:
        for a in [z] + geom + [pos]:
            f.write(np.ascontiguousarray(a).tobytes())
    out = os.path.join(work, "out.bin")
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.pathsep.join([os.path.join(REPO, "brushstroke_engine_amd", "csrc"), "/opt/rocm/lib",
                                              env.get("LD_LIBRARY_PATH", "")])
    r = subprocess.run([exe, "128", mode, str(n), os.path.join(work, "weights.bin"), os.path.join(work, "inputs.bin"), out], env=env,
                       capture_output=True, text=True, timeout=300)
    print(r.stdout + r.stderr, flush=True)
    check(r.returncode == 0, f"generate exited with {r.returncode}")
    ng = NativeGenerator.from_state_dict(cfg, sd, mode, n, DEV)
    u8, _, dbg = ng.render_triad(z=D(z), geom_feature=[D(g) for g in geom], positions=D(pos))
    want = np.concatenate([u8.cpu().numpy().reshape(-1).view(np.uint8), dbg["uvs"].cpu().numpy().reshape(-1).view(np.uint8),
                           dbg["colors"].cpu().numpy().reshape(-1).view(np.uint8)])
    got = np.fromfile(out, dtype=np.uint8)
    check(got.size == 2 * want.size, f"out.bin size {got.size}, expected {2 * want.size}")
    check(np.array_equal(got[:want.size], want), "C host eager == NativeGenerator")
    check(np.array_equal(got[want.size:], want), "C host graph replay == NativeGenerator")
    ng.close()


if __name__ == "__main__":
    case = sys.argv[1]
    torch.cuda.set_device(0)
    torch.set_num_threads(min(16, torch.get_num_threads()))        # (the CPU oracle)
    if case == "packers":
        packers()
    elif case == "python":
        python_vs_c(sys.argv[2], int(sys.argv[3]))
    elif case == "matrix":
        matrix(sys.argv[2], sys.argv[3])
    elif case == "oracle":
        oracle(sys.argv[2])
    elif case == "golden":
        golden(sys.argv[2])
    elif case == "graph":
        graph(sys.argv[2], int(sys.argv[3]))
    elif case == "chost":
        chost(sys.argv[2], sys.argv[3])
    else:
        raise SystemExit(f"unknown case {case}")
    print("[capi] done", flush=True)
