"""Child process of tests/test_hip_capi_staged.py: one group of checks of the staged C generator entry (nb_generator_forward_staged,
nb_generator_describe_staged) and the canvas helpers of a C host (nb_dirty_area_alpha_f32) on the GPU.

    python tests/_capi_staged_worker.py python <mode> <R>    # head / tail == the Python _stop_after / _resume passes, bitwise
    python tests/_capi_staged_worker.py errors               # the error cases on a real handle: nothing written
    python tests/_capi_staged_worker.py graph                # captured head / tail == eager, also after the inputs change in place
    python tests/_capi_staged_worker.py alpha                # nb_dirty_area_alpha_f32 == painting.dirty_area_alpha, bitwise
    python tests/_capi_staged_worker.py paint <exe> <workdir> <mode> <level>   # examples/capi/paint_blended.c == PaintingHelper

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
from _capi_geom_worker import D, DEV, check, masks  # noqa: E402


def perturbed(x, seed):
    """The head's output with a seeded perturbation: what the blend hands the tail is not the whole pass's own value."""
    gen = torch.Generator(device=x.device).manual_seed(seed)
    return (x + 0.25 * torch.randn(x.shape, generator=gen, device=x.device) * x.abs().mean()).contiguous()


def new_outputs(n, r):
    return {"rgba_u8": torch.zeros([n, r, r, 4], dtype=torch.uint8, device=DEV), "uvs": torch.zeros([n, 3, r, r], device=DEV),
            "colors": torch.zeros([n, 3, 3], device=DEV)}


def python_vs_c(mode, R, stages, batches):
    cfg = cfgmod.style1_config(R)
    G = Generator(cfg, wmod.random_state_dict(cfg, seed=5), conv_mode=mode).to(DEV)
    G.sub_stream_min_batch = 10 ** 9                          # the Python pass as one chain too
    ng = NativeGenerator.from_generator(G, n_max=max(batches))
    esd = encmod.random_encoder_state_dict(5)
    enc = encmod.HipGeometryEncoder(esd, "-11inverse")
    enc.arith = "f8" if mode == "f8" else "h3"                 # TileOps' rule
    ng.attach_encoder(esd, "-11inverse")
    kernels = G.synthesis.layer_kernels
    torgb = cfg.torgb_name
    for n in batches:
        z = D(synthetic.batch_z(cfg, n, 100 + n).astype(np.float32))
        ws = G.mapping(z, None).contiguous()
        feats_g = [D(g) for g in synthetic.geom_features(cfg, n, seed=n)]
        mask = D(masks(n, R, 7 * n))
        pos = D(synthetic.positions(cfg, n, seed=n))
        for res in stages:
            C = cfg.channels(res)
            for from_masks in (False, True):
                for positional in (True, False):
                    p = pos if positional else None
                    tag = f"{mode} R={R} n={n} res={res} {'masks' if from_masks else 'features'} positions {positional}"
                    # the latent: z through the mapping with stroke masks, pre-mapped ws with fp32 features (both input forms)
                    lat = dict(z=z) if from_masks else dict(ws=ws)
                    pgeom = (lambda: enc.lazy(mask)) if from_masks else (lambda: feats_g)
                    cgeom = dict(geom=mask) if from_masks else dict(geom_feature=feats_g)
                    # ---- head ----
                    kernels.clear()
                    if from_masks:
                        want = G(z, None, pgeom(), positions=p, noise_mode="const", _stop_after=res)
                    else:
                        want = G.forward_pre_mapped(ws, pgeom(), positions=p, noise_mode="const", _stop_after=res)
                    got = torch.full([n, C, res, res], 7.0, device=DEV)
                    ng.head(n, res, got, positions=p, **lat, **cgeom)
                    torch.cuda.synchronize()
                    if not torch.equal(want, got):
                        print(f"  head max |diff| {float((want - got).abs().max()):.3e}", flush=True)
                    check(torch.equal(want, got), f"{tag}: head == forward_pre_mapped(_stop_after), bitwise")
                    # (the Python head at R on the large kernels runs the fused ToRGB as a by-product; the C head has none)
                    pk = {k: v for k, v in kernels.items() if k != torgb}
                    check(ng.describe(n, stop_res=res) == pk, f"{tag}: describe(stop_res) == layer_kernels")
                    # ---- tail ----
                    x = perturbed(want, 1000 * n + res)
                    kernels.clear()
                    u8, _, dbg = G.render_triad(geom_feature=pgeom(), positions=p, _resume=(res, x), **lat)
                    outs = new_outputs(n, R)
                    if res > max(cfg.geom_feature_resolutions):        # no feature is read: none given
                        tgeom = {}
                    elif from_masks:
                        tgeom = cgeom
                    else:                                               # only the features at resolutions >= res
                        tgeom = dict(geom_feature=[g if r >= res else None for g, r in zip(feats_g, cfg.geom_feature_resolutions)])
                    ng.tail(n, res, x, outs, positions=p, **lat, **tgeom)
                    torch.cuda.synchronize()
                    same = torch.equal(u8, outs["rgba_u8"]) and torch.equal(dbg["uvs"], outs["uvs"]) and torch.equal(dbg["colors"], outs["colors"])
                    if not same:
                        print(f"  tail u8 {int((u8.int() - outs['rgba_u8'].int()).abs().max())} uvs {float((dbg['uvs'] - outs['uvs']).abs().max()):.3e} "
                              f"colors {float((dbg['colors'] - outs['colors']).abs().max()):.3e}", flush=True)
                    check(same, f"{tag}: tail == render_triad(_resume), bitwise")
                    check(ng.describe(n, resume_res=res) == dict(kernels), f"{tag}: describe(resume_res) == layer_kernels")
    ng.close()


def python_case(mode, R):
    if R == 128:
        python_vs_c(mode, R, (R, R // 2, R // 4), (1, 5, 8))
    else:                       # the large kernels, the operand hand-off and in-kernel noise
        python_vs_c(mode, R, (R // 2,), (1, 32))


def errors():
    cfg = cfgmod.style1_config(128)
    R, n = 128, 2
    ng = NativeGenerator.from_state_dict(cfg, wmod.random_state_dict(cfg, seed=1), "f8", 4, DEV)
    lib = _lib.lib()
    z = D(synthetic.batch_z(cfg, 8, 1).astype(np.float32))
    geom = [D(g) for g in synthetic.geom_features(cfg, 8, seed=1)]
    fout = torch.full([8, cfg.channels(64), 64, 64], 7.0, device=DEV)
    fin32 = torch.randn([8, cfg.channels(32), 32, 32], device=DEV)
    outs = {"uvs": torch.full([8, 3, R, R], 7.0, device=DEV), "rgba_u8": torch.full([8, R, R, 4], 7, dtype=torch.uint8, device=DEV)}

    def case(what, fn, want, msg):
        try:
            fn()
            rc = 0
        except _lib.NeubeHipError as e:
            rc = int(str(e).split("(")[1].split(")")[0])
        torch.cuda.synchronize()
        err = lib.nb_last_error().decode()
        clean = bool((outs["uvs"] == 7.0).all()) and bool((outs["rgba_u8"] == 7).all()) and bool((fout == 7.0).all())
        check(rc == want and msg in err and clean, f"{what}: code {rc}, nothing written ({err})")

    ins = _lib.NbGeneratorInputs()
    ins.z, ins.truncation_psi = z.data_ptr(), 1.0
    ins.geom[0], ins.geom[1] = geom[0].data_ptr(), geom[1].data_ptr()
    o = _lib.NbGeneratorOutputs()
    o.uvs = outs["uvs"].data_ptr()
    head = _lib.NbGeneratorStage(64, 0, fout.data_ptr(), None)
    case("an output pointer given to a head",
         lambda: _lib.check(lib.nb_generator_forward_staged(ng._h, ctypes.byref(ins), None, ctypes.byref(head), ctypes.byref(o), n, None), "fs"),
         _lib.NB_EINVAL, "every output pointer must be NULL")
    case("NULL features_out", lambda: ng.head(n, 64, None, z=z[:n], geom_feature=[g[:n] for g in geom]), _lib.NB_EINVAL, "null features_out")
    case("NULL features_in", lambda: ng.tail(n, 64, None, outs, z=z[:n]), _lib.NB_EINVAL, "null features_in")
    case("a resolution above R", lambda: ng.head(n, 256, fout, z=z[:n], geom_feature=geom), _lib.NB_EINVAL, "256 is not a block resolution")
    case("a tail at R/4 without its feature and without masks", lambda: ng.tail(n, 32, fin32, outs, z=z[:n], geom_feature=[geom[0], None]),
         _lib.NB_EINVAL, "geometry feature 1 is NULL")
    case("a tail at R/4 from masks without an encoder", lambda: ng.tail(n, 32, fin32, outs, z=z[:n], geom=D(masks(n, R, 1))),
         _lib.NB_EINVAL, "no encoder attached")
    case("a head without geometry", lambda: ng.head(n, 64, fout, z=z[:n]), _lib.NB_EINVAL, "geometry feature 0 is NULL")
    case("n > n_max (head)", lambda: ng.head(5, 64, fout, z=z[:5], geom_feature=geom), _lib.NB_EINVAL, "outside [1, n_max = 4]")
    case("n > n_max (tail)", lambda: ng.tail(5, 64, fout, outs, z=z[:5]), _lib.NB_EINVAL, "outside [1, n_max = 4]")
    case("NULL z and ws", lambda: ng.tail(n, 64, fout, outs), _lib.NB_EINVAL, "exactly one of z / ws")
    case("random noise (head)", lambda: ng.head(n, 64, fout, z=z[:n], geom_feature=geom, noise_mode="random"), _lib.NB_EUNSUPPORTED, "noise_mode 2")
    case("random noise (tail)", lambda: ng.tail(n, 64, fout, outs, z=z[:n], noise_mode="random"), _lib.NB_EUNSUPPORTED, "noise_mode 2")
    rc = lib.nb_generator_describe_staged(ng._h, 5, 64, 0, ctypes.create_string_buffer(4096), 4096)
    check(rc == _lib.NB_EINVAL and "outside [1, n_max = 4]" in lib.nb_last_error().decode(), f"describe_staged at n > n_max: {rc}")
    rc = lib.nb_generator_describe_staged(ng._h, 1, 0, 256, ctypes.create_string_buffer(4096), 4096)
    check(rc == _lib.NB_EINVAL and "256 is not a block resolution" in lib.nb_last_error().decode(), f"describe_staged above R: {rc}")
    ng.close()


def graph():
    mode, R = "f8", 256
    res = R // 2
    cfg = cfgmod.style1_config(R)
    sd = wmod.random_state_dict(cfg, seed=9)
    esd = encmod.random_encoder_state_dict(5)
    C = cfg.channels(res)
    for n in (1, 32):
        ng = NativeGenerator.from_state_dict(cfg, sd, mode, n, DEV)
        ng.attach_encoder(esd, "-11inverse")
        z = D(synthetic.batch_z(cfg, n, 11).astype(np.float32))
        pos = D(synthetic.positions(cfg, n, seed=11))
        mask = D(masks(n, R, 11))
        # ---- head (from stroke masks) ----
        eager, out = torch.zeros([n, C, res, res], device=DEV), torch.zeros([n, C, res, res], device=DEV)
        ng.head(n, res, eager, z=z, geom=mask, positions=pos)               # eager: also sets the kernels' attributes
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            ng.head(n, res, out, z=z, geom=mask, positions=pos)
        gr.replay()
        torch.cuda.synchronize()
        check(torch.equal(out, eager), f"head n={n}: graph replay == eager")
        mask2, z2 = D(masks(n, R, 12)), D(synthetic.batch_z(cfg, n, 12).astype(np.float32))
        mask.copy_(mask2)
        z.copy_(z2)
        gr.replay()
        want = torch.zeros_like(out)
        ng.head(n, res, want, z=z2, geom=mask2, positions=pos)
        torch.cuda.synchronize()
        check(torch.equal(out, want) and not torch.equal(want, eager), f"head n={n}: replay after the inputs changed in place == eager on the new inputs")
        del gr
        # ---- tail ----
        x = perturbed(want, n)
        eager, outs = new_outputs(n, R), new_outputs(n, R)
        ng.tail(n, res, x, eager, z=z, positions=pos)
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            ng.tail(n, res, x, outs, z=z, positions=pos)
        gr.replay()
        torch.cuda.synchronize()
        check(all(torch.equal(outs[k], eager[k]) for k in outs), f"tail n={n}: graph replay == eager")
        x2 = perturbed(want, n + 100)
        x.copy_(x2)
        pos.copy_(D(synthetic.positions(cfg, n, seed=12)))
        gr.replay()
        want_t = new_outputs(n, R)
        ng.tail(n, res, x2, want_t, z=z, positions=pos)
        torch.cuda.synchronize()
        check(all(torch.equal(outs[k], want_t[k]) for k in outs) and not torch.equal(want_t["uvs"], eager["uvs"]),
              f"tail n={n}: replay after the inputs changed in place == eager on the new inputs")
        del gr
        ng.close()


def alpha():
    lib = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    # the engine's own templates (R = 128 and 256, levels 1..3, crop margin 10, blend margin 16: painting.py _schedule) and three more
    triples = [(R // df, 16 // df, 10 // df) for R in (128, 256) for df in (1, 2, 4)] + [(16, 1, 0), (100, 7, 3), (512, 16, 10)]
    for width, margin, crop in triples:
        got = torch.full([width * width + 64], -3.0, device=DEV)
        _lib.check(lib.nb_dirty_area_alpha_f32(got.data_ptr(), width, margin, crop, st), "dirty_area_alpha")
        torch.cuda.synchronize()
        want = painting.dirty_area_alpha(width, margin, crop)
        g = got.cpu().numpy()
        same = np.array_equal(g[:width * width].reshape(width, width).view(np.uint32), want.view(np.uint32))
        check(same and bool((g[width * width:] == -3.0).all()), f"alpha0 ({width}, {margin}, {crop}) == painting.dirty_area_alpha, bitwise")
    buf = torch.full([64 * 64], -3.0, device=DEV)
    for width, margin, crop, msg in [(64, 0, 5, "bad sizes"), (64, 22, 10, "leave no interior")]:
        rc = lib.nb_dirty_area_alpha_f32(buf.data_ptr(), width, margin, crop, st)
        torch.cuda.synchronize()
        check(rc == _lib.NB_EINVAL and msg in lib.nb_last_error().decode() and bool((buf == -3.0).all()),
              f"alpha0 ({width}, {margin}, {crop}): NB_EINVAL, nothing written")


def paint(exe, work, mode, level):
    from conftest import load_golden
    g = load_golden("engine_r128.npz")
    cfg = cfgmod.style1_config(128)
    R, m, batch = 128, int(g["crop_margin"]), 4
    sd, esd = wmod.random_state_dict(cfg, seed=0), encmod.random_encoder_state_dict(5)
    z = np.random.RandomState(594).randn(1, cfg.z_dim).astype(np.float32)
    # ---- the Python engine ----
    G = Generator(cfg, sd, conv_mode=mode).to(DEV)
    helper = painting.PaintingHelper(painting.TileOps(G, encmod.HipGeometryEncoder(esd)), batch=batch)
    helper.set_feature_blending(level)
    opts = painting.GanBrushOptions()
    opts.set_style(torch.from_numpy(z), 594)
    _, full, crops, padded = helper.paint_image(g["geom"], opts, crop_margin=m, return_full=True)
    want_f, want_m = helper.features[0].cpu().numpy(), helper.mask.cpu().numpy()
    # ---- the C program ----
    yx = np.array([c[:2] for c in crops], np.int32)
    H, W = padded.shape[:2]
    with open(os.path.join(work, "weights.bin"), "wb") as f:
        for name, _ in param_table(cfg):
            f.write(np.ascontiguousarray(np.asarray(sd[name], np.float32)).tobytes())
    with open(os.path.join(work, "encoder.bin"), "wb") as f:
        for name, _ in encoder_param_table():
            f.write(np.ascontiguousarray(np.asarray(esd[name], np.float32)).tobytes())
    with open(os.path.join(work, "job.bin"), "wb") as f:
        f.write(np.array([H, W, len(yx), m], np.int32).tobytes() + np.ascontiguousarray(padded[..., 0]).tobytes() + yx.tobytes() + z.tobytes()
                + np.array([helper.feature_blending_margin], np.int32).tobytes())
    out = os.path.join(work, "out.bin")
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.pathsep.join([os.path.join(REPO, "brushstroke_engine_amd", "csrc"), "/opt/rocm/lib", env.get("LD_LIBRARY_PATH", "")])
    r = subprocess.run([exe, str(R), mode, str(batch), os.path.join(work, "weights.bin"), os.path.join(work, "encoder.bin"), "0", str(level),
                        os.path.join(work, "job.bin"), out], env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout + r.stderr, flush=True)
    check(r.returncode == 0, f"paint_blended exited with {r.returncode}")
    df = 2 ** (level - 1)
    C, hc, wc = cfg.channels(R // df), -(-H // df), -(-W // df)
    got = np.fromfile(out, np.uint8)
    check(got.size == H * W * 4 + C * hc * wc * 4 + hc * wc, f"out.bin size {got.size}")
    canvas = got[:H * W * 4].reshape(H, W, 4)
    fcanvas = got[H * W * 4:H * W * 4 + C * hc * wc * 4].view(np.float32).reshape(C, hc, wc)
    mask = got[H * W * 4 + C * hc * wc * 4:].reshape(hc, wc)
    check(want_f.shape == fcanvas.shape and want_m.shape == mask.shape, f"feature canvas {fcanvas.shape}, mask {mask.shape}")
    if not np.array_equal(full, canvas):
        d = np.abs(full.astype(np.int32) - canvas.astype(np.int32))
        print(f"  canvas: {(d > 0).sum()} bytes differ, max {d.max()}; features max |diff| {np.abs(want_f - fcanvas).max():.3e}", flush=True)
    check(np.array_equal(want_m, mask), f"{mode} level {level}: mask == PaintingHelper's, bitwise")
    check(np.array_equal(want_f.view(np.uint32), fcanvas.view(np.uint32)), f"{mode} level {level}: feature canvas == PaintingHelper's, bitwise")
    check(np.array_equal(full, canvas), f"{mode} level {level}: canvas == PaintingHelper's, bitwise")
    if level == 2:
        # the reference engine's canvas: the bounds of tests/test_hip_painting.py (_canvas_close; test_tiled_canvas_matches_reference)
        d = np.abs(canvas.astype(np.int32) - g["canvas_level2_clear"].astype(np.int32))
        frac = float((d > 0).mean())
        fd = float(np.abs(fcanvas[::16, ::4, ::4] - g["feature_canvas_sub"]).max())
        print(f"[capi staged paint {mode}] vs canvas_level2_clear: max {int(d.max())}, {frac:.2e} of the bytes differ; "
              f"vs feature_canvas_sub: max |diff| {fd:.3e}", flush=True)
        check(d.max() <= 1 and frac <= (5e-3 if mode == "f8" else 1e-3), f"{mode} paint_blended.c canvas within the reference bounds")
        np.testing.assert_allclose(fcanvas[::16, ::4, ::4], g["feature_canvas_sub"], atol={"h3": 1e-4, "f32": 2e-5, "f8": 2e-3}[mode])
        check(True, f"{mode} paint_blended.c feature canvas within the reference bound")
        check(float(mask.sum()) == g["feature_canvas_stats"][2], "mask count == the reference's")


if __name__ == "__main__":
    case = sys.argv[1]
    torch.cuda.set_device(0)
    if case == "python":
        python_case(sys.argv[2], int(sys.argv[3]))
    elif case == "errors":
        errors()
    elif case == "graph":
        graph()
    elif case == "alpha":
        alpha()
    elif case == "paint":
        paint(sys.argv[2], sys.argv[3], sys.argv[4], int(sys.argv[5]))
    else:
        raise SystemExit(f"unknown case {case}")
    print("[capi staged] done", flush=True)
