"""Child process of tests/test_hip_capi_brush_noise.py: brush noise sets through the C generator (nb_brush_noise_create / _load /
_destroy, nb_generator_bind_brush_noise) on the GPU.

    python tests/_capi_brush_noise_worker.py python <mode>   # create -> load -> bind -> forward == the Python pass on the same set
    python tests/_capi_brush_noise_worker.py binding         # unloaded set, bind(NULL), describe, another handle's set, destroy

Prints one line per check and exits non-zero at the first failure (the parent shows the output)."""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

from brushstroke_engine_amd import _lib, config as cfgmod, encoder as encmod, synthetic, weights as wmod  # noqa: E402
from brushstroke_engine_amd.native import NativeGenerator  # noqa: E402
from brushstroke_engine_amd.networks import Generator  # noqa: E402
from _capi_geom_worker import D, DEV, check, masks  # noqa: E402

R, N = 64, 4          # style1 R=64 at batch 4: large kernels with in-kernel noise, the fused styles + noise launch


def buffers(cfg, seed):
    rs = np.random.RandomState(seed)
    return {f"b{s.block_res}.conv{0 if s.up == 2 else 1}.noise_const": rs.randn(s.block_res, s.block_res).astype(np.float32)
            for s in cfg.layers}


def triad_equal(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[2]["uvs"], b[2]["uvs"]) and torch.equal(a[2]["colors"], b[2]["colors"])


def new_outputs(n, r):
    return {"rgba_u8": torch.zeros([n, r, r, 4], dtype=torch.uint8, device=DEV), "uvs": torch.zeros([n, 3, r, r], device=DEV),
            "colors": torch.zeros([n, 3, 3], device=DEV)}


def python_vs_c(mode):
    cfg = cfgmod.style1_config(R)
    G = Generator(cfg, wmod.random_state_dict(cfg, seed=5), conv_mode=mode).to(DEV)
    G.sub_stream_min_batch = 10 ** 9                          # the Python pass as one chain too
    ng = NativeGenerator.from_generator(G, n_max=N)
    esd = encmod.random_encoder_state_dict(5)
    enc = encmod.HipGeometryEncoder(esd, "-11inverse")
    enc.arith = "f8" if mode == "f8" else "h3"                 # TileOps' rule
    ng.attach_encoder(esd, "-11inverse")
    A, B = buffers(cfg, 41), buffers(cfg, 42)
    z = D(synthetic.batch_z(cfg, N, 100).astype(np.float32))
    ws = G.mapping(z, None).contiguous()
    geom = [D(g) for g in synthetic.geom_features(cfg, N, seed=3)]
    mask = D(masks(N, R, 7))
    pos = D(synthetic.positions(cfg, N, seed=3))
    plain = G.render_triad(ws=ws, geom_feature=geom, positions=pos)
    pset, cset = G.synthesis.brush_noise(), ng.brush_noise()
    ng.bind_brush_noise(cset)
    # (alpha 0.25: the same weights from a C float and from a Python float)
    for what, load in (("load(A)", lambda s: s.load(A)), ("load(A, B, 0.25)", lambda s: s.load(A, other=B, alpha=0.25)),
                       ("load(b8.* only)", lambda s: s.load({k: v for k, v in A.items() if k.startswith("b8.")}))):
        load(pset)
        load(cset)
        tag = f"{mode} {what}"
        for positional in (True, False):
            p = pos if positional else None
            want = G.render_triad(ws=ws, geom_feature=geom, positions=p, noise_set=pset)
            check(triad_equal(ng.render_triad(ws=ws, geom_feature=geom, positions=p), want),
                  f"{tag} positions {positional}: nb_generator_forward == render_triad(noise_set), bitwise")
        shown = G.render_triad(ws=ws, geom_feature=geom, positions=pos, noise_set=pset)
        check(not torch.equal(shown[2]["uvs"], plain[2]["uvs"]), f"{tag}: the set's noise is what was rendered")
        want = G.render_triad(z=z, geom_feature=enc.lazy(mask), positions=pos, noise_set=pset)
        check(triad_equal(ng.render_triad(z=z, geom=mask, positions=pos), want), f"{tag}: nb_generator_forward_geom == render_triad(noise_set), bitwise")
        res = R // 2
        head = G.forward_pre_mapped(ws, geom, positions=pos, noise_mode="const", _stop_after=res, noise_set=pset).clone()
        got = torch.full_like(head, 7.0)
        ng.head(N, res, got, ws=ws, geom_feature=geom, positions=pos)
        torch.cuda.synchronize()
        check(torch.equal(got, head), f"{tag}: staged head == forward_pre_mapped(_stop_after, noise_set), bitwise")
        x = (head * 0.75 - 0.02).contiguous()
        tail = G.render_triad(ws=ws, geom_feature=geom, positions=pos, _resume=(res, x), noise_set=pset)
        outs = new_outputs(N, R)
        ng.tail(N, res, x, outs, ws=ws, geom_feature=geom, positions=pos)
        torch.cuda.synchronize()
        check(torch.equal(outs["rgba_u8"], tail[0]) and torch.equal(outs["uvs"], tail[2]["uvs"]) and torch.equal(outs["colors"], tail[2]["colors"]),
              f"{tag}: staged tail == render_triad(_resume, noise_set), bitwise")
    # the other noise modes ignore the binding
    none = ng.render_triad(ws=ws, geom_feature=geom, positions=pos, noise_mode="none")
    ng.bind_brush_noise(None)
    check(triad_equal(none, ng.render_triad(ws=ws, geom_feature=geom, positions=pos, noise_mode="none")), f"{mode}: noise_mode none ignores the set")
    cset.close()
    ng.close()


def binding():
    cfg = cfgmod.style1_config(R)
    sd = wmod.random_state_dict(cfg, seed=5)
    ng = NativeGenerator.from_state_dict(cfg, sd, "f8", N, DEV)
    other = NativeGenerator.from_state_dict(cfg, sd, "f8", N, DEV)
    lib = _lib.lib()
    ws = D(np.random.RandomState(1).randn(N, cfg.num_ws, cfg.w_dim).astype(np.float32))
    geom = [D(g) for g in synthetic.geom_features(cfg, N, seed=3)]
    pos = D(synthetic.positions(cfg, N, seed=3))
    call = lambda: ng.render_triad(ws=ws, geom_feature=geom, positions=pos)       # noqa: E731
    unbound, lines = call(), ng.describe(N)
    bn = ng.brush_noise()
    ng.bind_brush_noise(bn)
    check(triad_equal(call(), unbound), "a bound but unloaded set == an unbound forward, bitwise")
    check(ng.describe(N) == lines and ng.describe(N, stop_res=32) == NativeGenerator.describe(other, N, stop_res=32),
          "nb_generator_describe is unchanged by the binding")
    bn.load(buffers(cfg, 41))
    loaded = call()
    check(not torch.equal(loaded[0], unbound[0]), "a loaded set changes the picture")
    ng.bind_brush_noise(None)
    check(triad_equal(call(), unbound), "bind(NULL) restores the unbound result, bitwise")
    rc = lib.nb_generator_bind_brush_noise(other._h, bn._h)
    check(rc == _lib.NB_EINVAL and b"another generator" in lib.nb_last_error(), f"a set of another handle: code {rc} ({lib.nb_last_error().decode()})")
    check(triad_equal(NativeGenerator.render_triad(other, ws=ws, geom_feature=geom, positions=pos), unbound), "... and binds nothing")
    ng.bind_brush_noise(bn)
    check(triad_equal(call(), loaded), "bound again: the loaded set, bitwise")
    bn.close()
    check(triad_equal(call(), unbound), "destroying a bound set unbinds it")
    other.close()
    ng.close()


if __name__ == "__main__":
    what = sys.argv[1]
    if what == "python":
        python_vs_c(sys.argv[2])
    elif what == "binding":
        binding()
    else:
        raise SystemExit(f"unknown check {what!r}")
    print("[capi brush noise] done", flush=True)
