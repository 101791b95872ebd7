"""What the stitching scores cost: R = 256, margin 10 (S = 226), an ``alex`` of the full widths with seeded random weights --

  (a) pairs         ``stitch_pairs`` on n = 16 samples (32 raw images that are already there) on the kernel of
                    csrc/nb_stitch_metrics.hip against the float32 torch restatement of ``TileOpsBase`` on the same device tensors
                    (it composites sample by sample on the host's schedule, which is what a torch caller of per-unit rectangles
                    does), and against a device copy that moves the same number of bytes (``copy_`` of (bytes in + bytes out) / 2);
  (b) evaluate      a whole ``BrushEvaluator.evaluate`` of a seed library with ``lpips`` and with ``lpips`` and ``stitch``, the
                    full-size drawings being the guidance drawings padded to D = 384.

Everything is warmed, then alternated within this process for --repeats rounds; every time is the host clock around work that ends in
a device synchronise, the pairs and the copy as --inner back-to-back calls per measurement, divided.

    python tools/bench_stitch_metrics.py [--repeats 5] [--brushes 12] [--out profiles/stitch_metrics_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from brushstroke_engine_amd import build, config as cfgmod, encoder as encmod, formats, metrics, painting, perceptual  # noqa: E402
from brushstroke_engine_amd import tile_ops  # noqa: E402
from brushstroke_engine_amd import weights as wmod  # noqa: E402
from bench_catalogue import calibration_drawings  # noqa: E402
from bench_perceptual_metrics import alex_weights, stats  # noqa: E402

R, MARGIN, MIN_OVERLAP, N_PAIRS, D_FULL = 256, 10, 50, 16, 384


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--brushes", type=int, default=12)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--conv-mode", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    build.build(verbose=False)
    if not torch.cuda.is_available():
        raise SystemExit("bench_stitch_metrics needs a GPU: a CPU run says nothing about kernels or launches")
    from brushstroke_engine_amd.networks import DEFAULT_CONV_MODE, Generator
    dev = torch.device("cuda:0")
    cfg = cfgmod.style1_config(R)
    mode = a.conv_mode or DEFAULT_CONV_MODE
    G = Generator(cfg, wmod.random_state_dict(cfg, seed=0), conv_mode=mode).to(dev)
    enc = encmod.HipGeometryEncoder(encmod.random_encoder_state_dict(5), device=dev)
    drawings = calibration_drawings(R)[0]
    k = int(drawings.shape[0])
    full = np.full((k, D_FULL, D_FULL), 255, np.uint8)
    full[:, 64:64 + R, 64:64 + R] = drawings
    setup = metrics.StitchSetup(full, MARGIN, MIN_OVERLAP)
    library = formats.SeedBrushLibrary(list(range(a.brushes)), cfg.z_dim)
    net = perceptual.LPIPS(alex_weights(), route="hip", device=dev)
    ops = {"kernel": painting.TileOps(G, enc), "restated": painting.TileOpsBase()}
    with torch.no_grad():
        evaluator = metrics.BrushEvaluator(ops["kernel"], drawings)

    # (a) the pairs: images as a generator pass leaves them, rectangles of a plan's crop pairs (one pair per sample)
    s = R - 3 * MARGIN
    plan = metrics.default_stitch_plan(0, N_PAIRS, 1, 1, R, D_FULL, MARGIN, MIN_OVERLAP)
    rects = [tile_ops.stitch_rects((*plan["crop1"][i, 0], R, R), (*plan["crop2"][i, 0], R, R), MARGIN) for i in range(N_PAIRS)]
    ra = torch.from_numpy(np.stack([q[0] for q in rects])).to(dev)
    rb = torch.from_numpy(np.stack([q[1] for q in rects])).to(dev)
    fake = torch.tanh(torch.randn([2 * N_PAIRS, 3, R, R], generator=torch.Generator().manual_seed(0))).to(dev)
    bytes_in, bytes_out = fake.numel() * 4, 4 * N_PAIRS * 3 * s * s * 4
    src = torch.empty([(bytes_in + bytes_out) // 8], dtype=torch.float32, device=dev).normal_()
    dst = torch.empty_like(src)

    def pairs(name):
        for _ in range(a.inner):
            out = ops[name].stitch_pairs(fake, ra, rb, MARGIN)
        torch.cuda.synchronize()
        return out

    def copy(name):
        for _ in range(a.inner):
            dst.copy_(src)
        torch.cuda.synchronize()

    def evaluate(name):
        out = evaluator.evaluate(library, batch=a.batch, lpips=net, stitch=setup if name == "with_stitch" else None)
        torch.cuda.synchronize()
        return out

    def timed(fn, name, per=1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn(name)
        return (time.perf_counter() - t0) * 1e3 / per, out

    groups = {"pairs": (pairs, ("kernel", "restated"), a.inner), "copy": (copy, ("same_bytes",), a.inner),
              "evaluate": (evaluate, ("with_stitch", "without_stitch"), 1)}
    with torch.no_grad():
        for _, (fn, names, _) in groups.items():                           # warm-up: workspaces, code objects, the caching allocator
            for name in names:
                fn(name), fn(name)
        times = {f"{w}_{n}": [] for w, (_, names, _) in groups.items() for n in names}
        last = {}
        for _ in range(a.repeats):
            for w, (fn, names, per) in groups.items():
                for name in names:
                    ms, last[f"{w}_{name}"] = timed(fn, name, per)
                    times[f"{w}_{name}"].append(ms)
    res = {"bench": "stitch_metrics", "device": torch.cuda.get_device_name(0), "conv_mode": mode, "resolution": R, "margin": MARGIN, "crop_width": s,
           "pairs_samples": N_PAIRS, "pairs_bytes_in": bytes_in, "pairs_bytes_out": bytes_out, "inner": a.inner, "brushes": a.brushes, "drawings": k,
           "full_size": D_FULL, "batch": a.batch, "repeats": a.repeats, "lpips_net": "alex"}
    for name, v in times.items():
        res[name] = stats(v)
    gbs = lambda ms: round((bytes_in + bytes_out) / (ms * 1e-3) / 1e9, 1)
    res["pairs_kernel_gb_per_s"], res["copy_gb_per_s"] = gbs(res["pairs_kernel"]["median_ms"]), gbs(res["copy_same_bytes"]["median_ms"])
    res["pairs_kernel_over_copy"] = round(res["pairs_kernel"]["median_ms"] / max(res["copy_same_bytes"]["median_ms"], 1e-9), 2)
    res["pairs_ratio"] = round(res["pairs_restated"]["median_ms"] / max(res["pairs_kernel"]["median_ms"], 1e-9), 2)
    spread = max(res[f"pairs_{n}"]["max_ms"] - res[f"pairs_{n}"]["min_ms"] for n in ("kernel", "restated"))
    res["pairs_gain_ms"] = round(res["pairs_restated"]["median_ms"] - res["pairs_kernel"]["median_ms"], 3)
    res["pairs_spread_ms"], res["pairs_faster_beyond_spread"] = round(spread, 3), bool(res["pairs_gain_ms"] > spread)
    res["evaluate_stitch_cost_ms"] = round(res["evaluate_with_stitch"]["median_ms"] - res["evaluate_without_stitch"]["median_ms"], 3)
    res["evaluate_stitch_cost_per_brush_ms"] = round(res["evaluate_stitch_cost_ms"] / max(a.brushes, 1), 3)
    kx, kl = last["pairs_kernel"]                                           # faster must not mean different
    rx, rl = last["pairs_restated"]
    res["pairs_same_bytes"] = bool(torch.equal(kx, rx))
    res["max_rel_diff_l1"] = float(((kl - rl).abs() / rl.abs().clamp(min=1e-30)).max())
    for key in metrics.KEYS + metrics.PERCEPTUAL_KEYS:
        x, y = last["evaluate_with_stitch"].as_dict()[key], last["evaluate_without_stitch"].as_dict()[key]
        res[f"same_bits_{key}"] = bool(x.tobytes() == y.tobytes())
    for key in metrics.STITCH_KEYS:
        res[f"summary_{key}"] = float(np.mean(last["evaluate_with_stitch"].stitching[key]))
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return res


if __name__ == "__main__":
    main()
