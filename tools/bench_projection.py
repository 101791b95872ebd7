"""What a step of the brush projection costs: ``projection.BrushProjector`` on ``training.TrainableGenerator``, ``style1_config(256)``
with synthetic weights, B = 10 patches per exemplar, K = 1 and K = 4 exemplars per pass, W+ and noise planes, ``with_composite`` over
the mean background colour, both weights positive, no perceptual item --

  (a) step           ms per whole step (generator forward and backward, loss, regulariser, Adam + renormalisation) with
                     ``route="hip"`` (csrc/nb_projection.hip, csrc/nb_clarity.hip) and ``route="torch"`` (the reference's operations in
                     float32 torch) on the same device tensors;
  (b) non_generator  the part the kernels replace, alone: loss forward + backward on fixed uvs / colors tensors, regulariser value +
                     gradient, Adam + renormalisation -- the generator stubbed out -- both ways.

Everything is warmed, then the two routes alternate within this process for --repeats rounds of --steps steps; every time is the host
clock around work that ends in a device synchronise.  The gradient arenas of the two routes from the same state are compared, so that
faster does not mean different.  No threshold is set: the generator dominates the step; the figures say whether the kernels win on
the part outside it.

    python tools/bench_projection.py [--repeats 5] [--steps 5] [--out profiles/projection_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from brushstroke_engine_amd import build, clarity, config as cfgmod, encoder as encmod, projection, weights as wmod  # noqa: E402
from bench_catalogue import calibration_drawings  # noqa: E402

R, B = 256, 10
WEIGHTS = dict(l1_fg_weight=1.0, bg_weight=0.5)


def stats(t):
    return {"median_ms": round(float(np.median(t)), 3), "min_ms": round(min(t), 3), "max_ms": round(max(t), 3), "all_ms": [round(x, 3) for x in t]}


def exemplars(k, seed=0):
    """K exemplars of B patches, each with drawings of its own: calibration drawings, a paper colour outside the stroke and a textured ink inside."""
    rs = np.random.RandomState(seed)
    pool = calibration_drawings(R, k=k * B)[1]                             # the thick ones, 24 pixels wide, every drawing another curve
    out = []
    for i in range(k):
        geom = (pool[i * B:(i + 1) * B].astype(np.float32) / 255.0)[:, None]
        paper, ink = rs.uniform(0.7, 0.95, [1, 3, 1, 1]), rs.uniform(0.05, 0.4, [1, 3, 1, 1])
        target = np.clip(geom * paper + (1 - geom) * (ink + 0.05 * rs.randn(B, 3, R, R)), 0, 1).astype(np.float32)
        out.append((torch.from_numpy(target), torch.from_numpy(geom), None, None))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5, help="steps per timed window")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    build.build(verbose=False)
    if not torch.cuda.is_available():
        raise SystemExit("bench_projection needs a GPU: a CPU run says nothing about kernels or launches")
    from brushstroke_engine_amd.training import TrainableGenerator
    dev = torch.device("cuda:0")
    cfg = cfgmod.style1_config(R)
    T = TrainableGenerator(cfg, wmod.random_state_dict(cfg, seed=0), dev).requires_grad_(False).eval()
    enc = encmod.HipGeometryEncoder(encmod.random_encoder_state_dict(5), device=dev)
    projs = {r: projection.BrushProjector(T, enc.encode, route=r, w_plus=True, with_composite=True, w_avg=np.zeros([1, 1, cfg.w_dim], np.float32), w_std=1.0,
                                          **WEIGHTS) for r in ("hip", "torch")}
    lo = projs["hip"].layout
    weights = projs["hip"].weights
    res = {"bench": "projection", "device": torch.cuda.get_device_name(0), "resolution": R, "patches": B, "repeats": a.repeats, "steps": a.steps,
           "planes": len(lo.res), "row_floats": lo.p, "with_composite": True, **WEIGHTS}
    for k in (1, 4):
        gen = torch.Generator().manual_seed(k)
        exs = exemplars(k)
        fix = {r: projs[r].prepare(exs) for r in projs}
        res[f"k{k}_counts_fg_bg"] = fix["hip"]["counts_host"].tolist()
        assert np.array_equal(fix["hip"]["counts_host"], fix["torch"]["counts_host"]) and fix["hip"]["counts_host"].min() > 0
        arena0 = torch.randn([k, lo.p], generator=gen).to(dev)
        w_noise = (0.05 * torch.randn([k, *lo.w_shape], generator=gen)).to(dev)
        hip_ops = clarity.HipArenaOps(lo, k, dev)
        uvs = torch.softmax(torch.randn([k * B, 3, R, R], generator=gen).to(dev), dim=1)
        colors = torch.tanh(torch.randn([k * B, 3, 3], generator=gen)).to(dev)
        state = {r: [arena0.clone(), torch.zeros_like(arena0), torch.zeros_like(arena0)] for r in projs}

        def step(route, n_steps):
            arena, m, v = state[route]
            for i in range(n_steps):
                grad = projs[route].loss_and_grad(arena, w_noise, fix[route], hip_ops if route == "hip" else None)[0]
                if route == "hip":
                    hip_ops.step(arena, grad, m, v, 0.01, i + 1)
                else:
                    clarity.step_torch(arena, grad, m, v, lo, 0.01, i + 1)
            torch.cuda.synchronize()

        def non_generator(route, n_steps):
            arena, m, v = state[route]
            f = fix[route]
            for i in range(n_steps):
                u, c = uvs.detach().requires_grad_(True), colors.detach().requires_grad_(True)
                if route == "hip":
                    total, _, _ = projection.fused_projection_loss(u, c, None, f["target"], None, f["bg_color"], f["mask"], f["counts"], k, True, weights)
                    total.sum().backward()
                    grad = torch.zeros_like(arena)
                    hip_ops.noise_reg(arena, grad, 10.0)
                    hip_ops.step(arena, grad, m, v, 0.01, i + 1)
                else:
                    x = arena.detach().requires_grad_(True)
                    total = projection.loss_torch(u, c, None, f["target"], None, f["bg_color"], f["fg"], f["bg"], k, True, weights)[0][:, 2]
                    (total.sum() + 10.0 * clarity.noise_reg_torch(x, lo).sum()).backward()
                    clarity.step_torch(arena, x.grad, m, v, lo, 0.01, i + 1)
            torch.cuda.synchronize()

        def timed(fn, route):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(route, a.steps)
            return (time.perf_counter() - t0) * 1e3 / a.steps

        grads = {r: projs[r].loss_and_grad(arena0, w_noise, fix[r], hip_ops if r == "hip" else None)[0] for r in projs}
        res[f"k{k}_max_abs_diff_grad"] = float((grads["hip"] - grads["torch"]).abs().max())
        res[f"k{k}_max_abs_grad"] = float(grads["torch"].abs().max())
        for fn in (step, non_generator):                                   # warm-up: code objects, workspaces, the caching allocator
            for r in projs:
                fn(r, 2)
        times = {f"{w}_{r}": [] for w in ("step", "non_generator") for r in projs}
        for _ in range(a.repeats):
            for w, fn in (("step", step), ("non_generator", non_generator)):
                for r in projs:
                    times[f"{w}_{r}"].append(timed(fn, r))
        for name, t in times.items():
            res[f"k{k}_{name}"] = stats(t)
        for w in ("step", "non_generator"):
            spread = max(res[f"k{k}_{w}_{r}"]["max_ms"] - res[f"k{k}_{w}_{r}"]["min_ms"] for r in projs)
            res[f"k{k}_{w}_gain_ms"] = round(res[f"k{k}_{w}_torch"]["median_ms"] - res[f"k{k}_{w}_hip"]["median_ms"], 3)
            res[f"k{k}_{w}_spread_ms"] = round(spread, 3)
            res[f"k{k}_{w}_hip_faster_beyond_spread"] = bool(res[f"k{k}_{w}_gain_ms"] > spread)
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return res


if __name__ == "__main__":
    main()
