"""Synthetic drawings in batches against the routes they replace, on the same box in the same process.

  batch      SplineSynth.batch(K): counts on the host, then nb_synth_spline_ctrl_f32 + nb_spline_flatten_f32 + nb_raster_batch_u8;
  host       what a tool without the sampler does today: strokes.raster_strokes_numpy per drawing on the host (the curves are taken
             as given: the time of sampling them is not counted) plus the upload of the [K,R,R] uint8 stack;
  per_call   K calls of TileOps.raster_strokes, one drawing each (two uploads, a flatten and a raster launch per drawing);
  one_launch TileOps.raster_strokes_batch on the same K stroke lists (two uploads, one flatten, one raster launch).

Every route includes host work, so the clock is the host's around `--inner` repetitions that end in a device synchronise; the routes
alternate, medians of --runs windows after a warm-up, with the spread.  The host route runs once per window (it takes seconds).
The outputs are compared before anything is timed: per_call == one_launch == batch byte for byte, host within the band.

    python tools/bench_drawings.py [--runs 7] [--inner 10] [--out profiles/drawings_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from brushstroke_engine_amd import build, config as cfgmod, drawings as dr, encoder as encmod, painting, weights as wmod  # noqa: E402
from brushstroke_engine_amd.strokes import raster_strokes_numpy  # noqa: E402

R, KS, SEED = 256, (32, 256), 1


def window(fn, inner, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3 / inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    build.build(verbose=False)
    if not torch.cuda.is_available():
        raise SystemExit("bench_drawings needs a GPU: a CPU run says nothing about kernels or copies")
    dev = torch.device("cuda:0")
    from brushstroke_engine_amd.networks import Generator
    cfg = cfgmod.style1_config(128)                                   # (raster_strokes needs an ops; the networks play no part)
    ops = painting.TileOps(Generator(cfg, wmod.random_state_dict(cfg, seed=0), conv_mode="h3").to(dev),
                           encmod.HipGeometryEncoder(encmod.random_encoder_state_dict(5)))
    synth = dr.SplineSynth(dr.SplineSpec(mode="cells"), R, SEED, dev)
    rows = []
    for k in KS:
        lists = [synth.strokes(i) for i in range(k)]
        uploaded = torch.empty([k, R, R], dtype=torch.uint8, device=dev)
        keep = {}

        def batch():
            keep["batch"] = synth.batch(k)

        def host():
            stack = np.stack([raster_strokes_numpy(s, (R, R)) for s in lists])
            uploaded.copy_(torch.from_numpy(stack), non_blocking=True)

        def per_call():
            keep["per_call"] = [ops.raster_strokes(s, (R, R)) for s in lists]

        def one_launch():
            keep["one_launch"] = ops.raster_strokes_batch(lists, (R, R))

        fns = {"batch": batch, "host": host, "per_call": per_call, "one_launch": one_launch}
        for fn in fns.values():                                       # warm-up, and the outputs to compare
            fn()
        torch.cuda.synchronize(dev)
        assert torch.equal(torch.stack(keep["per_call"]), keep["one_launch"]) and torch.equal(keep["batch"], keep["one_launch"])
        differ = float((uploaded != keep["batch"]).float().mean())
        assert differ <= 0.002, differ
        times = {name: [] for name in fns}
        for _ in range(a.runs):
            for name, fn in fns.items():
                times[name].append(window(fn, 1 if name == "host" else a.inner, dev))
        med = {name: float(np.median(v)) for name, v in times.items()}
        segs, seg_off = synth.segments(k)
        row = {"k": k, "r": R, "segments": int(seg_off[-1]), "stroke_pixel_share": round(float((keep["batch"] == 0).float().mean()), 4),
               "host_differs_share": differ, **{f"{name}_ms": round(v, 4) for name, v in med.items()},
               "host_over_batch": round(med["host"] / med["batch"], 2), "per_call_over_one_launch": round(med["per_call"] / med["one_launch"], 2),
               "spread_ms": {name: [round(min(v), 4), round(max(v), 4)] for name, v in times.items()}}
        rows.append(row)
        print(json.dumps(row), flush=True)
    res = {"bench": "drawings", "runs": a.runs, "inner": a.inner, "device": torch.cuda.get_device_name(0), "rows": rows}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return res


if __name__ == "__main__":
    main()
