"""The C generator entry (nb_generator_forward, via native.NativeGenerator) next to the Python paths on the same box:
batch-1 graph replay (p50 / p99 per replay, host clock around replay + synchronise) against GraphedTriadRender, and a batch-32
R=256 step (mean over a loop, one synchronise at the end) against single-stream Generator.render_triad.

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
    print(res)


if __name__ == "__main__":
    main()
