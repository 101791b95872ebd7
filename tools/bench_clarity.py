"""What a step of the clarity optimisation costs: ``clarity.ClarityOptimizer`` on ``training.TrainableGenerator``, ``style1_config(256)``
with synthetic weights, batch 20, K = 1 and K = 4 brushes per pass --

  (a) step           ms per whole step (encoder, two generator passes, backward, loss, regulariser, Adam + renormalisation) with
                     ``route="hip"`` (csrc/nb_clarity.hip) and ``route="torch"`` (the reference's operations in float32 torch) on the same
                     device tensors;
  (b) non_generator  the part the kernels replace, alone: loss forward + backward on fixed uvs / image / target tensors, regulariser
                     value + gradient, Adam + renormalisation -- the generator stubbed out -- both ways.

Everything is warmed, then the two routes alternate within this process for --repeats rounds of --steps steps; every time is the host
clock around work that ends in a device synchronise.  The gradient arenas of the two routes from the same state are compared, so that
faster does not mean different.  No threshold is set: the figures say whether the kernels win.

    python tools/bench_clarity.py [--repeats 5] [--steps 5] [--out profiles/clarity_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from brushstroke_engine_amd import build, clarity, config as cfgmod, encoder as encmod, weights as wmod  # noqa: E402
from bench_catalogue import calibration_drawings  # noqa: E402

R, BATCH = 256, 20


def stats(t):
    return {"median_ms": round(float(np.median(t)), 3), "min_ms": round(min(t), 3), "max_ms": round(max(t), 3), "all_ms": [round(x, 3) for x in t]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5, help="steps per timed window")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    build.build(verbose=False)
    if not torch.cuda.is_available():
        raise SystemExit("bench_clarity needs a GPU: a CPU run says nothing about kernels or launches")
    from brushstroke_engine_amd.training import TrainableGenerator
    dev = torch.device("cuda:0")
    cfg = cfgmod.style1_config(R)
    T = TrainableGenerator(cfg, wmod.random_state_dict(cfg, seed=0), dev).requires_grad_(False).eval()
    enc = encmod.HipGeometryEncoder(encmod.random_encoder_state_dict(5), device=dev)
    drawings = np.concatenate([calibration_drawings(R)[0]] * 4)[:BATCH]
    assert drawings.shape == (BATCH, R, R)
    geom = (torch.from_numpy(drawings).to(dev).float() / 255).unsqueeze(1)
    opts = {r: clarity.ClarityOptimizer(T, enc.encode, drawings, route=r, w_std=1.0) for r in ("hip", "torch")}
    lo = opts["hip"].layout
    res = {"bench": "clarity", "device": torch.cuda.get_device_name(0), "resolution": R, "batch": BATCH, "repeats": a.repeats, "steps": a.steps,
           "planes": len(lo.res), "row_floats": lo.p}
    for k in (1, 4):
        gen = torch.Generator().manual_seed(k)
        arena0 = torch.randn([k, lo.p], generator=gen).to(dev)
        w_start = lo.w(arena0).clone()
        w_noise = (0.05 * torch.randn([k, *lo.w_shape], generator=gen)).to(dev)
        hip_ops = clarity.HipArenaOps(lo, k, dev)
        fixed = {n: torch.randn([k * BATCH, 3, R, R], generator=gen).to(dev) for n in ("uvs", "img", "target")}
        fixed["uvs"] = torch.softmax(fixed["uvs"], dim=1)
        state = {r: [arena0.clone(), torch.zeros_like(arena0), torch.zeros_like(arena0)] for r in opts}
        weights = opts["hip"].fused_weights

        def step(route, n_steps):
            arena, m, v = state[route]
            for i in range(n_steps):
                grad, _, _ = opts[route].loss_and_grad(arena, w_start, w_noise, geom, hip_ops if route == "hip" else None)
                if route == "hip":
                    hip_ops.step(arena, grad, m, v, 0.01, i + 1)
                else:
                    clarity.step_torch(arena, grad, m, v, lo, 0.01, i + 1)
            torch.cuda.synchronize()

        def non_generator(route, n_steps):
            arena, m, v = state[route]
            for i in range(n_steps):
                u, im = fixed["uvs"].detach().requires_grad_(True), fixed["img"].detach().requires_grad_(True)
                if route == "hip":
                    total, _ = clarity.fused_clarity_loss(u, im, fixed["target"], geom, k, weights)
                    total.sum().backward()
                    grad = torch.zeros_like(arena)
                    hip_ops.noise_reg(arena, grad, 10.0)
                    hip_ops.step(arena, grad, m, v, 0.01, i + 1)
                else:
                    x = arena.detach().requires_grad_(True)
                    total = clarity.loss_torch(u, im, fixed["target"], geom, k, weights)[:, 3]
                    (total.sum() + 10.0 * clarity.noise_reg_torch(x, lo).sum()).backward()
                    clarity.step_torch(arena, x.grad, m, v, lo, 0.01, i + 1)
            torch.cuda.synchronize()

        def timed(fn, route):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(route, a.steps)
            return (time.perf_counter() - t0) * 1e3 / a.steps

        grads = {r: opts[r].loss_and_grad(arena0, w_start, w_noise, geom, hip_ops if r == "hip" else None)[0] for r in opts}
        res[f"k{k}_max_abs_diff_grad"] = float((grads["hip"] - grads["torch"]).abs().max())
        res[f"k{k}_max_abs_grad"] = float(grads["torch"].abs().max())
        for fn in (step, non_generator):                                   # warm-up: code objects, workspaces, the caching allocator
            for r in opts:
                fn(r, 2)
        times = {f"{w}_{r}": [] for w in ("step", "non_generator") for r in opts}
        for _ in range(a.repeats):
            for w, fn in (("step", step), ("non_generator", non_generator)):
                for r in opts:
                    times[f"{w}_{r}"].append(timed(fn, r))
        for name, t in times.items():
            res[f"k{k}_{name}"] = stats(t)
        for w in ("step", "non_generator"):
            spread = max(res[f"k{k}_{w}_{r}"]["max_ms"] - res[f"k{k}_{w}_{r}"]["min_ms"] for r in opts)
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
