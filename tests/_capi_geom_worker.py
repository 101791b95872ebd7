"""Child process of tests/test_hip_capi_geom.py: one group of checks of the geometry encoder behind the C generator entry
(nb_generator_attach_encoder, nb_generator_forward_geom) on the GPU.

    python tests/_capi_geom_worker.py python <mode> <R>    # render_triad(geom=mask) == Generator.render_triad(lazy encoder), bitwise
    python tests/_capi_geom_worker.py errors               # the NB_EINVAL cases of attach and forward_geom on a real handle
    python tests/_capi_geom_worker.py graph <mode> <R>     # captured forward_geom == eager, also after the mask changes in place
    python tests/_capi_geom_worker.py paint <exe> <workdir> <mode>   # examples/capi/paint.c on the reference's level-0 canvas

Prints one line per check and exits non-zero at the first failure (the parent shows the output)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

from brushstroke_engine_amd import _lib, config as cfgmod, encoder as encmod, painting, synthetic, weights as wmod  # noqa: E402
from brushstroke_engine_amd.native import NativeGenerator, encoder_param_table, param_table  # noqa: E402
from brushstroke_engine_amd.networks import Generator  # noqa: E402

DEV = torch.device("cuda:0")
PREPROCS = (None, "-11inverse", "inverse")


def D(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def check(ok, what):
    print(("ok   " if ok else "FAIL ") + what, flush=True)
    if not ok:
        sys.exit(1)


def masks(n, r, seed):
    """Stroke patches [n, 1, r, r] (1 = background): background with strokes of every grey level, as nb_geom_tiles_f32 writes them."""
    rs = np.random.RandomState(seed)
    g = np.full((n, 1, r, r), 255, np.uint8)
    yy, xx = np.mgrid[0:r, 0:r]
    for i in range(n):
        for _ in range(3):
            cy, cx, rad = rs.uniform(0, r), rs.uniform(0, r), rs.uniform(r / 10, r / 3)
            g[i, 0][(yy - cy) ** 2 + (xx - cx) ** 2 < rad ** 2] = rs.randint(0, 200)
    g[:, :, ::7, ::5] = rs.randint(0, 256, g[:, :, ::7, ::5].shape)
    return (1.0 - (255.0 - g.astype(np.float32)) / np.float32(255.0)).astype(np.float32)


def ragged_encoder_state_dict(seed):
    """random_encoder_state_dict with BatchNorm statistics over several decades (tiny and huge variances, large means)."""
    sd = encmod.random_encoder_state_dict(seed)
    rs = np.random.RandomState(seed + 1)
    for k, v in sd.items():
        if k.endswith("running_var"):
            sd[k] = (10.0 ** rs.uniform(-4, 2, v.shape)).astype(np.float32)
        elif k.endswith("running_mean"):
            sd[k] = (rs.randn(*v.shape) * 3).astype(np.float32)
        elif k.endswith(".1.weight"):
            sd[k] = (rs.randn(*v.shape) * 0.5).astype(np.float32)
    return sd


def handoff_taken(G, n, positional):
    kp = G.synthesis.pass_plan(n, noise_positions=_lib.NB_PLAN_POS_INT if positional else _lib.NB_PLAN_POS_NONE)
    r1 = G.img_resolution // 4
    return bool(kp.geom[1].encoder_handoff) and (r1 % 32 == 0 or r1 == 16)


def python_vs_c(mode, res, batches):
    cfg = cfgmod.style1_config(res)
    G = Generator(cfg, wmod.random_state_dict(cfg, seed=5), conv_mode=mode).to(DEV)
    G.sub_stream_min_batch = 10 ** 9                          # the Python pass as one chain too
    ng = NativeGenerator.from_generator(G, n_max=max(batches))
    routes = set()
    for k, esd in enumerate((encmod.random_encoder_state_dict(5), ragged_encoder_state_dict(11))):
        for pre in PREPROCS:
            enc = encmod.HipGeometryEncoder(esd, pre)
            enc.arith = "f8" if mode == "f8" else "h3"         # TileOps' rule
            ng.attach_encoder(esd, pre)
            for n in batches:
                if k == 1 and n not in (batches[0], batches[-1]):
                    continue                                   # (the second weight set: the smallest and largest batch)
                z = D(synthetic.batch_z(cfg, n, 100 + n).astype(np.float32))
                mask = D(masks(n, res, 7 * n + k))
                pos = D(synthetic.positions(cfg, n, seed=n))
                for positional in (True, False):
                    kw = dict(z=z, positions=pos if positional else None)
                    u8, _, dbg = G.render_triad(geom_feature=enc.lazy(mask), **kw)
                    cu8, _, cdbg = ng.render_triad(geom=mask, **kw)
                    torch.cuda.synchronize()
                    same = torch.equal(u8, cu8) and torch.equal(dbg["uvs"], cdbg["uvs"]) and torch.equal(dbg["colors"], cdbg["colors"])
                    route = "hand-off" if handoff_taken(G, n, positional) else "fp32"
                    routes.add(route)
                    if not same:
                        print(f"  u8 {int((u8.int() - cu8.int()).abs().max())} uvs {float((dbg['uvs'] - cdbg['uvs']).abs().max()):.3e} "
                              f"colors {float((dbg['colors'] - cdbg['colors']).abs().max()):.3e}", flush=True)
                    check(same, f"{mode} R={res} weights {k} preproc {pre} n={n} positions {positional} ({route}): bitwise equal")
                check(ng.describe(n) == G.synthesis.layer_kernels, f"{mode} R={res} n={n}: describe == layer_kernels")
    print(f"[capi geom] {mode} R={res} feature-1 routes taken: {sorted(routes)}", flush=True)
    ng.close()
    return routes


def python_case(mode, res):
    batches = (1, 5, 7, 8, 16, 32) if res >= 128 else (1, 7, 8, 16)
    routes = python_vs_c(mode, res, batches)
    if mode == "f8" and res == 256:
        check("hand-off" in routes, "f8 R=256 takes the encoder's hand-off into the consumer's operands")
    if mode == "f32":
        check(routes == {"fp32"}, "f32 takes the fp32 route")


def errors():
    cfg = cfgmod.style1_config(128)
    n = 2
    ng = NativeGenerator.from_state_dict(cfg, wmod.random_state_dict(cfg, seed=1), "f8", 4, DEV)
    lib = _lib.lib()
    z, mask = D(synthetic.batch_z(cfg, n, 1).astype(np.float32)), D(masks(n, 128, 1))
    geom = [D(g) for g in synthetic.geom_features(cfg, n, seed=1)]
    outs = {"uvs": torch.full([8, 3, 128, 128], 7.0, device=DEV)}

    def code(fn):
        try:
            fn()
            return 0
        except _lib.NeubeHipError as e:
            return int(str(e).split("(")[1].split(")")[0])

    def forward_case(what, fn, want, msg):
        rc = code(fn)
        torch.cuda.synchronize()
        err = lib.nb_last_error().decode()
        check(rc == want and msg in err and bool((outs["uvs"] == 7.0).all()), f"{what}: code {rc}, nothing written ({err})")

    forward_case("no encoder attached", lambda: ng.forward_into(outs, n, z=z, geom=mask), _lib.NB_EINVAL, "no encoder attached")
    esd = encmod.random_encoder_state_dict(5)
    rc = code(lambda: _lib.check(lib.nb_generator_attach_encoder(ng._h, None, 3, None), "attach"))
    check(rc == _lib.NB_EINVAL and "unknown preproc" in lib.nb_last_error().decode(), f"attach with preproc 3: {rc}")
    ng.attach_encoder(esd, "inverse")
    ins, o = _lib.NbGeneratorInputs(), _lib.NbGeneratorOutputs()
    ins.z, ins.truncation_psi = z.data_ptr(), 1.0
    o.uvs = outs["uvs"].data_ptr()
    ins.geom[0], ins.geom[1] = geom[0].data_ptr(), geom[1].data_ptr()
    forward_case("geom and geom[] both given",
                 lambda: _lib.check(lib.nb_generator_forward_geom(ng._h, ctypes.byref(ins), mask.data_ptr(), ctypes.byref(o), n, None), "fg"),
                 _lib.NB_EINVAL, "geometry feature 0 given")
    ins.geom[0] = ins.geom[1] = None
    forward_case("NULL stroke patches", lambda: _lib.check(lib.nb_generator_forward_geom(ng._h, ctypes.byref(ins), None, ctypes.byref(o), n, None), "fg"),
                 _lib.NB_EINVAL, "null stroke patches")
    forward_case("n > n_max", lambda: _lib.check(lib.nb_generator_forward_geom(ng._h, ctypes.byref(ins), mask.data_ptr(), ctypes.byref(o), 5, None), "fg"),
                 _lib.NB_EINVAL, "outside [1, n_max = 4]")
    forward_case("NULL z and ws", lambda: ng.forward_into(outs, n, geom=mask), _lib.NB_EINVAL, "exactly one of z / ws")
    forward_case("random noise", lambda: ng.forward_into(outs, n, z=z, geom=mask, noise_mode="random"), _lib.NB_EUNSUPPORTED, "noise_mode 2")
    ng.close()
    # a generator whose geometry layout is not the encoder's
    from _gen_configs import CONFIGS
    cfg3 = CONFIGS["C3"][0]
    ng3 = NativeGenerator.from_state_dict(cfg3, wmod.random_state_dict(cfg3, seed=1), "h3", 2, DEV)
    rc = code(lambda: ng3.attach_encoder(esd))
    check(rc == _lib.NB_EINVAL and "geometry layout is not the encoder's" in lib.nb_last_error().decode(), f"attach to C3: {rc}")
    ng3.close()


def graph(mode, res):
    cfg = cfgmod.style1_config(res)
    sd = wmod.random_state_dict(cfg, seed=9)
    esd = encmod.random_encoder_state_dict(5)
    for n in (1, 32):
        ng = NativeGenerator.from_state_dict(cfg, sd, mode, n, DEV)
        ng.attach_encoder(esd, "-11inverse")
        z = D(synthetic.batch_z(cfg, n, 11).astype(np.float32))
        pos = D(synthetic.positions(cfg, n, seed=11))
        mask = D(masks(n, res, 11))
        r = res
        new = lambda: {"rgba_u8": torch.zeros([n, r, r, 4], dtype=torch.uint8, device=DEV), "uvs": torch.zeros([n, 3, r, r], device=DEV),
                       "colors": torch.zeros([n, 3, 3], device=DEV)}
        eager, outs = new(), new()
        ng.forward_into(eager, n, z=z, geom=mask, positions=pos)          # eager: also sets the kernels' attributes
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            ng.forward_into(outs, n, z=z, geom=mask, positions=pos)
        gr.replay()
        torch.cuda.synchronize()
        check(all(torch.equal(outs[k], eager[k]) for k in outs), f"{mode} R={res} n={n}: graph replay == eager")
        mask2 = D(masks(n, res, 12))
        mask.copy_(mask2)
        gr.replay()
        want = new()
        ng.forward_into(want, n, z=z, geom=mask2, positions=pos)
        torch.cuda.synchronize()
        check(all(torch.equal(outs[k], want[k]) for k in outs) and not torch.equal(want["uvs"], eager["uvs"]),
              f"{mode} R={res} n={n}: replay after the mask changed in place == eager on the new mask")
        del gr
        ng.close()


def paint(exe, work, mode):
    from conftest import load_golden
    g = load_golden("engine_r128.npz")
    cfg = cfgmod.style1_config(128)
    R, m, batch = 128, int(g["crop_margin"]), 4
    sd, esd = wmod.random_state_dict(cfg, seed=0), encmod.random_encoder_state_dict(5)
    z = np.random.RandomState(594).randn(1, cfg.z_dim).astype(np.float32)
    crops, padded = painting.generate_stitching_crops(painting.pad_geo(g["geom"][..., None] if g["geom"].ndim == 2 else g["geom"], m), R,
                                                      "all", 2 * m)
    check(np.array_equal(padded[..., 0], g["geom_padded"]), "the padded geometry of pad_geo / generate_stitching_crops == geom_padded")
    yx = np.array([c[:2] for c in crops], np.int32)
    H, W = padded.shape[:2]
    with open(os.path.join(work, "weights.bin"), "wb") as f:
        for name, _ in param_table(cfg):
            f.write(np.ascontiguousarray(np.asarray(sd[name], np.float32)).tobytes())
    with open(os.path.join(work, "encoder.bin"), "wb") as f:
        for name, _ in encoder_param_table():
            f.write(np.ascontiguousarray(np.asarray(esd[name], np.float32)).tobytes())
    with open(os.path.join(work, "job.bin"), "wb") as f:
        f.write(np.array([H, W, len(yx), m], np.int32).tobytes() + np.ascontiguousarray(g["geom_padded"]).tobytes() + yx.tobytes()
                + z.tobytes())
    out = os.path.join(work, "out.bin")
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.pathsep.join([os.path.join(REPO, "brushstroke_engine_amd", "csrc"), "/opt/rocm/lib", env.get("LD_LIBRARY_PATH", "")])
    r = subprocess.run([exe, str(R), mode, str(batch), os.path.join(work, "weights.bin"), os.path.join(work, "encoder.bin"), "0",
                        os.path.join(work, "job.bin"), out], env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout + r.stderr, flush=True)
    check(r.returncode == 0, f"paint exited with {r.returncode}")
    got = np.fromfile(out, np.uint8)
    check(got.size == H * W * 4 + 2 * R * R * 4, f"out.bin size {got.size}")
    canvas = got[:H * W * 4].reshape(H, W, 4)
    eager, replay = got[H * W * 4:H * W * 4 + R * R * 4], got[H * W * 4 + R * R * 4:]
    d = np.abs(canvas.astype(np.int32) - g["canvas_level0_clear"].astype(np.int32))
    frac = float((d > 0).mean())
    print(f"[capi geom paint {mode}] vs canvas_level0_clear: max {int(d.max())}, {frac:.2e} of the bytes differ", flush=True)
    check(d.max() <= 1 and frac <= (5e-3 if mode == "f8" else 1e-3), f"{mode} paint.c canvas within the reference bounds")
    check(np.array_equal(eager, replay), f"{mode} paint.c stroke graph replay == eager")
    # the same tiles through NativeGenerator.render_triad(geom=...) in the same batches, pasted as TileOps.paste does
    ng = NativeGenerator.from_state_dict(cfg, sd, mode, batch, DEV)
    ng.attach_encoder(esd, None)
    lib = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    gdev, yx_dev = D(g["geom_padded"]), D(yx)
    tiles = []
    for b0 in range(0, len(yx), batch):
        n = min(batch, len(yx) - b0)
        patches = torch.empty([n, 1, R, R], device=DEV)
        _lib.check(lib.nb_geom_tiles_f32(gdev.data_ptr(), H, W, yx_dev[b0:].data_ptr(), n, R, patches.data_ptr(), st), "geom_tiles")
        u8, _, _ = ng.render_triad(z=D(np.repeat(z, n, 0)), geom=patches, positions=D(yx[b0:b0 + n].astype(np.int64)))
        tiles.append(u8)
    tiles = torch.cat(tiles)
    want = torch.zeros([H, W, 4], dtype=torch.uint8, device=DEV)
    off, lst = painting.build_cells(np.concatenate([yx + m, yx + R - m], axis=1), H, W)
    off, lst = D(off), D(lst)                  # (kept alive: the launch reads them later)
    _lib.check(lib.nb_paste_tiles_u8(tiles.data_ptr(), len(yx), R, yx_dev.data_ptr(), m, want.data_ptr(), H, W, off.data_ptr(),
                                     lst.data_ptr(), st), "paste")
    wc = want.cpu().numpy()
    if not np.array_equal(wc, canvas):
        ys, xs, cs = np.nonzero(wc != canvas)
        print(f"  {ys.size} bytes differ, rows {ys.min()}..{ys.max()}, cols {xs.min()}..{xs.max()}, channels {sorted(set(cs.tolist()))}", flush=True)
        p1 = torch.empty([1, 1, R, R], device=DEV)
        _lib.check(lib.nb_geom_tiles_f32(gdev.data_ptr(), H, W, yx_dev.data_ptr(), 1, R, p1.data_ptr(), st), "geom_tiles")
        s1, _, _ = ng.render_triad(z=D(z), geom=p1, positions=D(yx[:1].astype(np.int64)))
        print(f"  stroke (tile 0, n=1) == paint.c's: {np.array_equal(s1.cpu().numpy().reshape(-1), eager)}; "
              f"tile 0 of the batch == paint.c's stroke: {np.array_equal(tiles[0].cpu().numpy().reshape(-1), eager)}", flush=True)
    check(np.array_equal(wc, canvas), f"{mode} paint.c canvas == NativeGenerator.render_triad(geom=...) + paste, bitwise")
    ng.close()


if __name__ == "__main__":
    case = sys.argv[1]
    torch.cuda.set_device(0)
    if case == "python":
        python_case(sys.argv[2], int(sys.argv[3]))
    elif case == "errors":
        errors()
    elif case == "graph":
        graph(sys.argv[2], int(sys.argv[3]))
    elif case == "paint":
        paint(sys.argv[2], sys.argv[3], sys.argv[4])
    else:
        raise SystemExit(f"unknown case {case}")
    print("[capi geom] done", flush=True)
