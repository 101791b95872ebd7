"""What the perceptual item costs: ``perceptual.LPIPS`` with the ``vgg`` trunk (synthetic weights of the real channel counts) at
R = 256 on 10 patches, forward and backward with respect to the second image, the target bound --

  (a) call      ms per whole call (one trunk pass forward, the head over five levels, and their backward) with ``route="hip"``
                (``ops.conv2d`` and csrc/nb_lpips.hip) and ``route="torch"`` (float32 torch operations) on the same device tensors;
  (b) non_conv  the part outside the convolutions, alone: the scaling layer, bias + ReLU + tap + pool and the head, forward and
                backward, on fixed convolution outputs -- the convolutions stubbed out -- both ways.

Everything is warmed, then the two routes alternate within this process for --repeats rounds of --steps calls; every time is the host
clock around work that ends in a device synchronise.  Values and gradients of the two routes are compared, so that faster does not
mean different.  No threshold is set: the numbers are reported as measured.

    python tools/bench_lpips.py [--repeats 5] [--steps 3] [--out profiles/lpips_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from brushstroke_engine_amd import build, ops, perceptual  # noqa: E402

R, N = 256, 10
CHANNELS = (64, 128, 256, 512, 512)


def stats(t):
    return {"median_ms": round(float(np.median(t)), 3), "min_ms": round(min(t), 3), "max_ms": round(max(t), 3), "all_ms": [round(x, 3) for x in t]}


def vgg_weights(seed=0):
    """He-scaled convolutions of vgg16's shapes, small biases, positive head weights: the arithmetic of the real network, not its values."""
    rs = np.random.RandomState(seed)
    out, c_in, level = {"arch": np.asarray("vgg")}, 3, 0
    for lay in perceptual.layer_plan("vgg"):
        c_out = CHANNELS[level]
        out[f"features.{lay.index}.weight"] = (rs.randn(c_out, c_in, 3, 3) * np.sqrt(2.0 / (9 * c_in))).astype(np.float32)
        out[f"features.{lay.index}.bias"] = (0.1 * rs.randn(c_out)).astype(np.float32)
        c_in = c_out
        if lay.level is not None:
            out[f"lin{level}.weight"] = (np.abs(rs.randn(c_out)) / c_out).astype(np.float32)
            level += 1
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=3, help="calls per timed window")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    build.build(verbose=False)
    if not torch.cuda.is_available():
        raise SystemExit("bench_lpips needs a GPU: a CPU run says nothing about kernels or launches")
    dev = torch.device("cuda:0")
    w = vgg_weights()
    nets = {r: perceptual.LPIPS(w, route=r, device=dev) for r in ("hip", "torch")}
    gen = torch.Generator().manual_seed(0)
    x0 = torch.tanh(torch.randn([N, 3, R, R], generator=gen)).to(dev)
    x1 = (x0 + 0.3 * torch.randn([N, 3, R, R], generator=gen).to(dev)).clamp(-1, 1)
    bound = {r: nets[r].bind(x0) for r in nets}
    K, hip = perceptual._HipKernels, nets["hip"]
    plan = hip.plan

    # fixed convolution outputs and stand-in gradients of the pooled maps for (b)
    with torch.no_grad():
        raws, x = [], K.scale(x1, hip.shift, hip.scale)
        for lay in plan:
            raws.append(ops.conv2d(x, hip.weights[lay.index], stride=1, padding=1))
            tap, pooled = K.relu_pool(raws[-1], hip.biases[lay.index], lay.window)
            x = pooled if lay.window else tap
        taps0 = hip.target_taps(x0)
        d_next = [1e-3 * torch.randn_like(F.max_pool2d(r, 2, 2) if lay.window else r) for r, lay in zip(raws, plan)]
        g = torch.ones([N], device=dev)

    def call(route, n_steps):
        for _ in range(n_steps):
            a1 = x1.detach().requires_grad_(True)
            bound[route](x0, a1).sum().backward()
        torch.cuda.synchronize()

    def non_conv(route, n_steps):
        for _ in range(n_steps):
            if route == "hip":
                acc = torch.zeros([N], device=dev)
                K.scale(x1, hip.shift, hip.scale)
                for raw, lay, dn in zip(raws, plan, d_next):
                    tap, _ = K.relu_pool(raw, hip.biases[lay.index], lay.window)
                    d_tap = None if lay.window else dn
                    if lay.level is not None:
                        kept = K.head(taps0[lay.level], tap, hip.lins[lay.level], acc)
                        d_tap = K.head_bwd(taps0[lay.level], tap, hip.lins[lay.level], kept, g, out=None if d_tap is None else d_tap.clone())
                    K.relu_pool_bwd(tap, d_tap, dn if lay.window else None, lay.window)
                K.scale(x1, None, hip.scale)
            else:
                net, total, leaves = nets["torch"], 0, []
                xs = x1.detach().requires_grad_(True)
                total = total + ((xs - net.shift.reshape(1, 3, 1, 1)) / net.scale.reshape(1, 3, 1, 1)).sum() * 0
                for raw, lay, dn in zip(raws, plan, d_next):
                    r = raw.detach().requires_grad_(True)
                    leaves.append(r)
                    y = F.relu(r + net.biases[lay.index].reshape(1, -1, 1, 1))
                    if lay.level is not None:
                        total = total + perceptual.head_torch(taps0[lay.level], y, net.lins[lay.level]).sum()
                    total = total + ((F.max_pool2d(y, 2, 2) if lay.window else y) * dn).sum()
                total.backward()
        torch.cuda.synchronize()

    def timed(fn, route):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(route, a.steps)
        return (time.perf_counter() - t0) * 1e3 / a.steps

    res = {"bench": "lpips", "device": torch.cuda.get_device_name(0), "arch": "vgg", "resolution": R, "patches": N, "repeats": a.repeats, "steps": a.steps}
    vals, grads = {}, {}
    for r in nets:
        a1 = x1.detach().requires_grad_(True)
        v = bound[r](x0, a1)
        v.sum().backward()
        vals[r], grads[r] = v.detach(), a1.grad
    res["values_hip"] = [float(x) for x in vals["hip"]]
    res["max_rel_diff_value"] = float(((vals["hip"] - vals["torch"]).abs() / vals["torch"].abs()).max())
    res["max_abs_diff_grad"], res["max_abs_grad"] = float((grads["hip"] - grads["torch"]).abs().max()), float(grads["torch"].abs().max())
    # the same with the trunk on the exact-fp32 conv kernels: what of the difference is the split-f16 products', what is ReLU and pool
    # decisions that rounding flips among the 177 M pre-activations (either route's, against the other)
    split, ops.TRAIN_SPLIT_F16 = ops.TRAIN_SPLIT_F16, False
    try:
        a1 = x1.detach().requires_grad_(True)
        v = bound["hip"](x0, a1)
        v.sum().backward()
    finally:
        ops.TRAIN_SPLIT_F16 = split
    res["fp32_convs_max_rel_diff_value"] = float(((v.detach() - vals["torch"]).abs() / vals["torch"].abs()).max())
    res["fp32_convs_max_abs_diff_grad"] = float((a1.grad - grads["torch"]).abs().max())
    for fn in (call, non_conv):                                            # warm-up: code objects, workspaces, the caching allocator
        for r in nets:
            fn(r, 2)
    times = {f"{w_}_{r}": [] for w_ in ("call", "non_conv") for r in nets}
    for _ in range(a.repeats):
        for w_, fn in (("call", call), ("non_conv", non_conv)):
            for r in nets:
                times[f"{w_}_{r}"].append(timed(fn, r))
    for name, t in times.items():
        res[name] = stats(t)
    for w_ in ("call", "non_conv"):
        spread = max(res[f"{w_}_{r}"]["max_ms"] - res[f"{w_}_{r}"]["min_ms"] for r in nets)
        res[f"{w_}_gain_ms"] = round(res[f"{w_}_torch"]["median_ms"] - res[f"{w_}_hip"]["median_ms"], 3)
        res[f"{w_}_spread_ms"] = round(spread, 3)
        res[f"{w_}_hip_faster_beyond_spread"] = bool(res[f"{w_}_gain_ms"] > spread)
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return res


if __name__ == "__main__":
    main()
