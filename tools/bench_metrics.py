"""What scoring a brush library costs: ``metrics.BrushEvaluator.evaluate`` on a 100-seed library at R = 256, default conv mode, five
guidance drawings, batch 32 (six brushes per generator pass) --

  (a) kernels      on ``TileOps``: ``nb_brush_metrics_f32`` and the selection launch per pass;
  (b) restated     the same evaluator, generator and selection, with ``eval_masks`` and ``brush_metrics`` replaced by the float32 torch
                   restatements of ``TileOpsBase`` on the same device tensors (the reference's ~25 launches per batch with full-size
                   temporaries);

and, apart from the generator, the scoring of one pass's 30 renders alone (``score_renders`` on renders that are already there),
both ways.  Everything is warmed, then alternated within this process for --repeats rounds; every time is the host clock around work
that ends in a device synchronise.  The scores of the last round are compared, so that faster does not mean different.

    python tools/bench_metrics.py [--repeats 5] [--brushes 100] [--out profiles/metrics_bench.json]

The kernels' own time comes from a separate ``rocprofv3 --kernel-trace --stats`` run of this tool (--repeats 1).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from brushstroke_engine_amd import build, config as cfgmod, encoder as encmod, formats, metrics, painting, weights as wmod  # noqa: E402
from bench_catalogue import calibration_drawings  # noqa: E402

R = 256


class RestatedOps(painting.TileOps):
    """``TileOps`` with the two metric operations taken from ``TileOpsBase``: torch on the device tensors."""
    eval_masks = painting.TileOpsBase.eval_masks
    brush_metrics = painting.TileOpsBase.brush_metrics


def stats(t):
    return {"median_ms": round(float(np.median(t)), 3), "min_ms": round(min(t), 3), "max_ms": round(max(t), 3), "all_ms": [round(x, 3) for x in t]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--brushes", type=int, default=100)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--conv-mode", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    build.build(verbose=False)
    if not torch.cuda.is_available():
        raise SystemExit("bench_metrics needs a GPU: a CPU run says nothing about kernels or launches")
    from brushstroke_engine_amd.networks import DEFAULT_CONV_MODE, Generator
    dev = torch.device("cuda:0")
    cfg = cfgmod.style1_config(R)
    mode = a.conv_mode or DEFAULT_CONV_MODE
    G = Generator(cfg, wmod.random_state_dict(cfg, seed=0), conv_mode=mode).to(dev)
    enc = encmod.HipGeometryEncoder(encmod.random_encoder_state_dict(5), device=dev)
    drawings = calibration_drawings(R)[0]
    library = formats.SeedBrushLibrary(list(range(a.brushes)), cfg.z_dim)
    with torch.no_grad():
        evs = {"kernels": metrics.BrushEvaluator(painting.TileOps(G, enc), drawings), "restated": metrics.BrushEvaluator(RestatedOps(G, enc), drawings)}
    kept = []

    def evaluate(name):
        s = evs[name].evaluate(library, batch=a.batch, on_pass=(lambda u, r, t: kept.append((r.clone(), t.clone()))) if not kept else None)
        torch.cuda.synchronize()
        return s

    def score(name):
        ren, tg = kept[0]
        out = evs[name].score_renders(ren, tg)
        torch.cuda.synchronize()
        return out

    def timed(fn, name):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn(name)
        return (time.perf_counter() - t0) * 1e3, out

    with torch.no_grad():
        for name in evs:                                                # warm-up: workspaces, code objects, the caching allocator
            evaluate(name), score(name), score(name)
        times = {f"{w}_{n}": [] for w in ("evaluate", "score_pass") for n in evs}
        last = {}
        for _ in range(a.repeats):
            for name in evs:
                ms, last[name] = timed(evaluate, name)
                times[f"evaluate_{name}"].append(ms)
            for name in evs:
                ms, last[f"pass_{name}"] = timed(score, name)
                times[f"score_pass_{name}"].append(ms)
    res = {"bench": "brush_metrics", "device": torch.cuda.get_device_name(0), "conv_mode": mode, "resolution": R, "brushes": a.brushes,
           "drawings": int(drawings.shape[0]), "batch": a.batch, "repeats": a.repeats, "pass_renders": int(kept[0][0].shape[0])}
    for name, t in times.items():
        res[name] = stats(t)
    for w in ("evaluate", "score_pass"):
        spread = max(res[f"{w}_{n}"]["max_ms"] - res[f"{w}_{n}"]["min_ms"] for n in evs)
        res[f"{w}_gain_ms"] = round(res[f"{w}_restated"]["median_ms"] - res[f"{w}_kernels"]["median_ms"], 3)
        res[f"{w}_spread_ms"] = round(spread, 3)
        res[f"{w}_kernels_faster_beyond_spread"] = bool(res[f"{w}_gain_ms"] > spread)
    for key in metrics.KEYS:
        x, y = last["kernels"].as_dict()[key].astype(np.float64), last["restated"].as_dict()[key].astype(np.float64)
        res[f"max_abs_diff_{key}"] = float(np.nanmax(np.abs(x - y)))
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return res


if __name__ == "__main__":
    main()
