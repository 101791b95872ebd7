"""What the perceptual brush scores cost: R = 256, five guidance drawings, batch 32 (six brushes per generator pass), an ``alex`` of
the full widths with seeded random weights (the timing does not depend on their values) --

  (a) prepare       the preparation of one pass's LPIPS inputs -- ``bg_mean_colors`` and ``metric_pairs`` for the masked windows and
                    ``metric_pairs`` for the across-drawing pairs, on 30 renders that are already there -- on the kernels of
                    csrc/nb_metric_patches.hip against the float32 torch restatements of ``TileOpsBase`` on the same device tensors;
                    ``bg_guidance`` (once per set of drawings) apart;
  (b) distance      ``LPIPS.pair_distance`` over the [2n,3,p,p] buffer (one trunk pass) against ``LPIPS.__call__`` on its two halves
                    (two trunk passes of n images);
  (c) evaluate      a whole ``BrushEvaluator.evaluate`` of a seed library with and without ``lpips``.

Everything is warmed, then alternated within this process for --repeats rounds; every time is the host clock around work that ends
in a device synchronise.  The restatement's offsets are those of one window pair per unit, as the evaluator's plan has them; it
slices window by window on the host's schedule, which is what a torch caller of per-unit windows does.

    python tools/bench_perceptual_metrics.py [--repeats 5] [--brushes 24] [--out profiles/perceptual_metrics_bench.json]
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
from brushstroke_engine_amd import weights as wmod  # noqa: E402
from bench_catalogue import calibration_drawings  # noqa: E402

R = 256
ALEX_WIDTHS = {0: 64, 3: 192, 6: 384, 8: 256, 10: 256}


def alex_weights(seed=0):
    """Seeded random weights of alexnet.features' shapes and a positive head."""
    rs = np.random.RandomState(seed)
    out, c_in = {"arch": np.asarray("alex")}, 3
    for level, (i, c_out) in enumerate(ALEX_WIDTHS.items()):
        k = perceptual.ARCHS["alex"]["kernels"].get(i, 3)
        out[f"features.{i}.weight"] = (rs.randn(c_out, c_in, k, k) * np.sqrt(2.0 / (c_in * k * k))).astype(np.float32)
        out[f"features.{i}.bias"] = (0.1 * rs.randn(c_out)).astype(np.float32)
        out[f"lin{level}.weight"] = np.abs(rs.randn(c_out)).astype(np.float32)
        c_in = c_out
    return out


def stats(t):
    return {"median_ms": round(float(np.median(t)), 3), "min_ms": round(min(t), 3), "max_ms": round(max(t), 3), "all_ms": [round(x, 3) for x in t]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--brushes", type=int, default=24)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--conv-mode", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    build.build(verbose=False)
    if not torch.cuda.is_available():
        raise SystemExit("bench_perceptual_metrics needs a GPU: a CPU run says nothing about kernels or launches")
    from brushstroke_engine_amd.networks import DEFAULT_CONV_MODE, Generator
    dev = torch.device("cuda:0")
    cfg = cfgmod.style1_config(R)
    mode = a.conv_mode or DEFAULT_CONV_MODE
    G = Generator(cfg, wmod.random_state_dict(cfg, seed=0), conv_mode=mode).to(dev)
    enc = encmod.HipGeometryEncoder(encmod.random_encoder_state_dict(5), device=dev)
    drawings = calibration_drawings(R)[0]
    k, p = int(drawings.shape[0]), metrics.default_patch_width(R)
    library = formats.SeedBrushLibrary(list(range(a.brushes)), cfg.z_dim)
    net = perceptual.LPIPS(alex_weights(), route="hip", device=dev)
    ops = {"kernels": painting.TileOps(G, enc), "restated": painting.TileOpsBase()}
    with torch.no_grad():
        evaluator = metrics.BrushEvaluator(ops["kernels"], drawings)
    kept = []

    def evaluate(name):
        first = not kept
        s = evaluator.evaluate(library, batch=a.batch, lpips=net if name == "with_lpips" else None,
                               on_pass=(lambda u, r, t, own_renders=None: kept.append(own_renders.clone())) if (first and name == "with_lpips") else None)
        torch.cuda.synchronize()
        return s

    nu = max(1, a.batch // k)
    plan = metrics.default_crops(0, nu, 1, k, R, p)
    t = lambda name, rep: torch.from_numpy(np.repeat(plan[name][:, 0], rep, 0).astype(np.int32)).to(dev).contiguous()
    off0, off1 = t("same_off0", k), t("same_off1", k)
    base = (torch.arange(nu, dtype=torch.int32, device=dev) * k).unsqueeze(1)
    perm, gperm = (base + t("same_perm", 1)).reshape(-1).contiguous(), (base + t("geo_perm", 1)).reshape(-1).contiguous()
    zero = torch.zeros([nu * k, 2], dtype=torch.int32, device=dev)
    geom = evaluator.masks.geom
    guidance = {}

    def guide(name):
        guidance[name] = ops[name].bg_guidance(geom)
        torch.cuda.synchronize()

    def prepare(name):
        o, ren, g = ops[name], kept[0], guidance[name]
        mean = o.bg_mean_colors(ren, g)
        x = o.metric_pairs(ren, g, mean, off0, off1, perm, p, True, True)
        y = o.metric_pairs(ren, None, None, zero, zero, gperm, R, False, False)
        torch.cuda.synchronize()
        return x, y

    pairs = {}

    def distance(name):
        x = pairs["x"]
        n = x.shape[0] // 2
        out = net.pair_distance(x) if name == "pair_distance" else net(x[:n], x[n:])
        torch.cuda.synchronize()
        return out

    def timed(fn, name):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn(name)
        return (time.perf_counter() - t0) * 1e3, out

    groups = {"evaluate": (evaluate, ("with_lpips", "without_lpips")), "guidance": (guide, tuple(ops)), "prepare": (prepare, tuple(ops)),
              "distance": (distance, ("pair_distance", "two_calls"))}
    with torch.no_grad():
        evaluate("with_lpips"), evaluate("without_lpips")                  # warm-up: workspaces, code objects, the caching allocator
        for name in ops:
            guide(name), prepare(name), prepare(name)
        pairs["x"] = prepare("kernels")[0]
        for name in groups["distance"][1]:
            distance(name), distance(name)
        times = {f"{w}_{n}": [] for w, (_, names) in groups.items() for n in names}
        last = {}
        for _ in range(a.repeats):
            for w, (fn, names) in groups.items():
                for name in names:
                    ms, last[f"{w}_{name}"] = timed(fn, name)
                    times[f"{w}_{name}"].append(ms)
    res = {"bench": "perceptual_metrics", "device": torch.cuda.get_device_name(0), "conv_mode": mode, "resolution": R, "patch_width": p,
           "brushes": a.brushes, "drawings": k, "batch": a.batch, "repeats": a.repeats, "pass_renders": int(kept[0].shape[0]), "lpips_net": "alex"}
    for name, v in times.items():
        res[name] = stats(v)
    for w, slow, fast in (("prepare", "restated", "kernels"), ("guidance", "restated", "kernels"), ("distance", "two_calls", "pair_distance")):
        spread = max(res[f"{w}_{n}"]["max_ms"] - res[f"{w}_{n}"]["min_ms"] for n in (slow, fast))
        res[f"{w}_gain_ms"] = round(res[f"{w}_{slow}"]["median_ms"] - res[f"{w}_{fast}"]["median_ms"], 3)
        res[f"{w}_ratio"] = round(res[f"{w}_{slow}"]["median_ms"] / max(res[f"{w}_{fast}"]["median_ms"], 1e-9), 2)
        res[f"{w}_spread_ms"] = round(spread, 3)
        res[f"{w}_faster_beyond_spread"] = bool(res[f"{w}_gain_ms"] > spread)
    res["evaluate_lpips_cost_ms"] = round(res["evaluate_with_lpips"]["median_ms"] - res["evaluate_without_lpips"]["median_ms"], 3)
    for i, what in enumerate(("masked_pairs", "across_pairs")):             # faster must not mean different
        res[f"max_abs_diff_{what}"] = float((last["prepare_kernels"][i] - last["prepare_restated"][i]).abs().max())
    res["max_abs_diff_distance"] = float((last["distance_pair_distance"] - last["distance_two_calls"]).abs().max())
    for key in metrics.KEYS:
        x, y = last["evaluate_with_lpips"].as_dict()[key], last["evaluate_without_lpips"].as_dict()[key]
        res[f"same_bits_{key}"] = bool(x.tobytes() == y.tobytes())
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return res


if __name__ == "__main__":
    main()
