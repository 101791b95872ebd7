"""The C generator entry (nb_generator_forward, via native.NativeGenerator) next to the Python paths on the same box:
batch-1 graph replay (p50 / p99 per replay, host clock around replay + synchronise) against GraphedTriadRender, and a batch-32
R=256 step (mean over a loop, one synchronise at the end) against single-stream Generator.render_triad.  The same two legs from
stroke masks (nb_generator_forward_geom, the encoder in the chain): batch 32 against TileOps.full on the lazy encoder, batch 1
against PaintingHelper.render_stroke's graph path.

    python tools/bench_capi.py [--mode f8] [--iters 400]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from brushstroke_engine_amd import build, config as cfgmod, synthetic, weights as wmod  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="f8")
    ap.add_argument("--iters", type=int, default=400)
    a = ap.parse_args()
    build.build(verbose=False)
    from brushstroke_engine_amd.graphed import GraphedTriadRender
    from brushstroke_engine_amd.native import NativeGenerator
    from brushstroke_engine_amd.networks import Generator
    dev = torch.device("cuda:0")
    cfg = cfgmod.style1_config(256)
    G = Generator(cfg, wmod.random_state_dict(cfg, 0), conv_mode=a.mode).to(dev)
    G.sub_stream_min_batch = 10 ** 9                       # one chain, as the C entry runs
    res = {"mode": a.mode}

    def pct(ts):
        ts = np.sort(np.asarray(ts) * 1e3)
        return float(np.percentile(ts, 50)), float(np.percentile(ts, 99))

    def inputs(n):
        return (torch.from_numpy(synthetic.batch_z(cfg, n, 0).astype(np.float32)).to(dev),
                [torch.from_numpy(g).to(dev) for g in synthetic.geom_features(cfg, n, 0)],
                torch.from_numpy(synthetic.positions(cfg, n, 0)).to(dev))

    # batch 1: graph replay
    z, geom, pos = inputs(1)
    gr = GraphedTriadRender(G, batch=1)
    gr.set_inputs(z=z, geom_feature=geom, positions=pos)
    ng = NativeGenerator.from_generator(G, n_max=32)
    r = cfg.img_resolution
    outs = {"rgba_u8": torch.empty([1, r, r, 4], dtype=torch.uint8, device=dev), "uvs": torch.empty([1, 3, r, r], device=dev),
            "img": torch.empty([1, 3, r, r], device=dev), "colors": torch.empty([1, 3, 3], device=dev)}
    ng.forward_into(outs, 1, z=z, geom_feature=geom, positions=pos)
    torch.cuda.synchronize()
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):
        ng.forward_into(outs, 1, z=z, geom_feature=geom, positions=pos)
    for name, fn in (("python_graph_b1", gr.replay), ("capi_graph_b1", cg.replay)):
        for _ in range(50):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.iters):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        p50, p99 = pct(ts)
        res[name] = {"p50_ms": round(p50, 4), "p99_ms": round(p99, 4)}
    torch.cuda.synchronize()
    assert torch.equal(gr.out_u8, outs["rgba_u8"]), "batch-1 graph outputs differ"
    # batch 32: eager steps on one stream
    n = 32
    z, geom, pos = inputs(n)
    steps = {"python_render_triad_b32": lambda: G.render_triad(z=z, geom_feature=geom, positions=pos),
             "capi_render_triad_b32": lambda: ng.render_triad(z=z, geom_feature=geom, positions=pos)}
    for name, fn in steps.items():
        for _ in range(20):
            fn()
        torch.cuda.synchronize()
        k = max(a.iters // 4, 20)
        t0 = time.perf_counter()
        for _ in range(k):
            fn()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / k
        res[name] = {"ms_per_step": round(dt * 1e3, 4), "patches_per_s": round(n / dt, 1)}
    mask_to_rgba(a, G, ng, cfg, dev, res, pct)
    print(res)


def mask_to_rgba(a, G, ng, cfg, dev, res, pct):
    """Stroke mask -> RGBA: the C chain (nb_generator_forward_geom) against the Python pass on the lazy encoder (TileOps.full, one
    chain) at batch 32, and a batch-1 graph replay of the C chain against PaintingHelper.render_stroke's graph path (whose time
    includes its host-side patch preparation and the copy of the RGBA tile to the host)."""
    from brushstroke_engine_amd import encoder as encmod, painting
    esd = encmod.random_encoder_state_dict(5)
    enc = encmod.HipGeometryEncoder(esd)
    ops = painting.TileOps(G, enc)                         # (sets the encoder's arithmetic by the generator's conv_mode)
    ng.attach_encoder(esd)
    r = cfg.img_resolution
    rs = np.random.RandomState(0)
    geo_u8 = np.full((r, r), 255, np.uint8)
    yy, xx = np.mgrid[0:r, 0:r]
    geo_u8[(yy - r / 2) ** 2 + (xx - r / 2) ** 2 < (r / 3) ** 2] = 0
    n = 32
    mask = torch.from_numpy(np.repeat((geo_u8 / np.float32(255)).astype(np.float32)[None, None], n, 0)).to(dev)
    z = torch.from_numpy(rs.randn(n, cfg.z_dim).astype(np.float32)).to(dev)
    pos = torch.from_numpy(rs.randint(0, 4096, (n, 2)).astype(np.int64)).to(dev)
    outs = {"rgba_u8": torch.empty([n, r, r, 4], dtype=torch.uint8, device=dev)}
    steps = {"python_mask_to_rgba_b32": lambda: ops.full(ops.map_style(z=z), ops.encode(mask), pos, "clear", None),
             "capi_mask_to_rgba_b32": lambda: ng.forward_into(outs, n, z=z, geom=mask, positions=pos)}
    for name, fn in steps.items():
        for _ in range(20):
            fn()
        torch.cuda.synchronize()
        k = max(a.iters // 4, 20)
        t0 = time.perf_counter()
        for _ in range(k):
            fn()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / k
        res[name] = {"ms_per_step": round(dt * 1e3, 4), "patches_per_s": round(n / dt, 1)}
    # batch 1: one interactive stroke from its mask
    o1 = {"rgba_u8": torch.empty([1, r, r, 4], dtype=torch.uint8, device=dev)}
    ng.forward_into(o1, 1, z=z[:1], geom=mask[:1], positions=pos[:1])
    torch.cuda.synchronize()
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):
        ng.forward_into(o1, 1, z=z[:1], geom=mask[:1], positions=pos[:1])
    helper = painting.PaintingHelper(ops)
    helper.make_new_canvas(r, r, feature_blending=0)
    opts = painting.GanBrushOptions()
    opts.set_style(torch.from_numpy(rs.randn(1, cfg.z_dim).astype(np.float32)), 0)
    opts.set_position(7, 11)
    stroke = (255 - geo_u8)[..., None]
    for name, fn in (("python_render_stroke_b1", lambda: helper.render_stroke(stroke, None, opts, meta={"x": 7, "y": 11})),
                     ("capi_mask_graph_b1", cg.replay)):
        for _ in range(50):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.iters):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        p50, p99 = pct(ts)
        res[name] = {"p50_ms": round(p50, 4), "p99_ms": round(p99, 4)}


if __name__ == "__main__":
    main()
