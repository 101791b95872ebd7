"""The stroke route into the painter against the two steps it replaces, on the same box in the same process.

  strokes   nb_spline_flatten_f32 + nb_raster_segments_u8 (clear = 1) from control points that are on the device already: spline
            strokes of 11 control points, 8 pieces per span, radii 1.5-4 px, spread over the canvas;
  raster    nb_raster_segments_u8 alone on the flattened rows;
  prepare   nb_geom_prepare_u8 on a gray uint8 drawing of the canvas' size (the raster's own output), already on the device;
  upload    a pinned host-to-device copy of that uint8 canvas.

HIP events around `--inner` back-to-back repetitions (a window of single launches would measure the launch), the four alternating,
medians of --runs windows after a warm-up.  Workloads: a 514 x 800 canvas with ~5 * 10^3 segments, 4096^2 with 10^4 and 10^5.

    python tools/bench_raster.py [--runs 9] [--inner 10] [--out profiles/raster_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from brushstroke_engine_amd import _lib, build, painting  # noqa: E402

WORKLOADS = [("lamali_sm", 514, 800, 5_000), ("4096_1e4", 4096, 4096, 10_000), ("4096_1e5", 4096, 4096, 100_000)]
POINTS, SUBDIV = 11, 8                       # 8 spans x 8 pieces = 64 segments per stroke


def synthetic_strokes(h, w, n_segments, seed=0):
    """(ctrl [P, 3] float32, stroke_off int32): random-walk splines inside the canvas, ~n_segments segments after flattening."""
    n_strokes = -(-n_segments // ((POINTS - 3) * SUBDIV))
    rs = np.random.RandomState(seed)
    step = max(h, w) / 40.0
    start = np.stack([rs.uniform(0, w, n_strokes), rs.uniform(0, h, n_strokes)], 1)[:, None, :]
    heading = np.cumsum(rs.uniform(-0.8, 0.8, (n_strokes, POINTS)), 1) + rs.uniform(0, 6.28, (n_strokes, 1))
    steps = rs.uniform(0.3, 1.0, (n_strokes, POINTS, 1)) * step * np.stack([np.cos(heading), np.sin(heading)], 2)
    pts = start + np.cumsum(steps, axis=1)
    rad = rs.uniform(1.5, 4.0, (n_strokes, POINTS, 1))
    ctrl = np.concatenate([pts, rad], 2).reshape(-1, 3).astype(np.float32)
    return ctrl, (np.arange(n_strokes + 1) * POINTS).astype(np.int32)


def window(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    build.build(verbose=False)
    if not torch.cuda.is_available():
        raise SystemExit("bench_raster needs a GPU: a CPU run says nothing about kernels or copies")
    dev = torch.device("cuda:0")
    lib = _lib.lib()
    stream = torch.cuda.current_stream(dev).cuda_stream
    rows = []
    for name, h, w, n_target in WORKLOADS:
        ctrl, off = synthetic_strokes(h, w, n_target)
        n_strokes = len(off) - 1
        n = int(lib.nb_spline_segment_count(ctrl.shape[0], n_strokes, SUBDIV))
        d_ctrl, d_off = torch.from_numpy(ctrl).to(dev), torch.from_numpy(off).to(dev)
        segs = torch.empty([n, painting.SEG_PITCH], dtype=torch.float32, device=dev)
        out = torch.empty([h, w], dtype=torch.uint8, device=dev)
        prepared = torch.empty([h, w], dtype=torch.uint8, device=dev)
        ws = torch.empty([_lib.NB_GEOM_PREP_WS_BYTES // 4], dtype=torch.int32, device=dev)
        host = torch.empty([h, w], dtype=torch.uint8).pin_memory()
        uploaded = torch.empty([h, w], dtype=torch.uint8, device=dev)

        def flatten():
            _lib.check(lib.nb_spline_flatten_f32(d_ctrl.data_ptr(), d_off.data_ptr(), ctrl.shape[0], n_strokes, SUBDIV, 0.5, segs.data_ptr(),
                                                 n, stream), "spline_flatten")

        def raster():
            _lib.check(lib.nb_raster_segments_u8(segs.data_ptr(), n, out.data_ptr(), h, w, 0, 0, 1, stream), "raster_segments")

        def strokes():
            flatten()
            raster()

        def prepare():
            _lib.check(lib.nb_geom_prepare_u8(out.data_ptr(), h, w, 1, prepared.data_ptr(), h, w, 0, 0, ws.data_ptr(), stream), "geom_prepare")

        def upload():
            uploaded.copy_(host, non_blocking=True)

        strokes()
        host.copy_(out)                                   # the rasterised canvas is the drawing the other two steps handle
        prepare()
        torch.cuda.synchronize(dev)
        assert torch.equal(prepared, out), "a two-valued drawing must come back from the Otsu threshold unchanged"
        stroke_share = float((out == 0).float().mean())
        fns = {"strokes": strokes, "raster": raster, "prepare": prepare, "upload": upload}
        times = {k: [] for k in fns}
        for k, fn in fns.items():                         # warm-up
            window(fn, 2)
        for _ in range(a.runs):
            for k, fn in fns.items():
                times[k].append(window(fn, a.inner))
        med = {k: float(np.median(v)) for k, v in times.items()}
        cells = -(-h // 64) * -(-w // 64)
        row = {"workload": name, "h": h, "w": w, "segments": n, "strokes": n_strokes, "stroke_pixel_share": round(stroke_share, 4),
               "cells": cells, "cull_tests": cells * n, "segment_bytes_read": cells * n * 32, "canvas_bytes": h * w,
               "strokes_ms": round(med["strokes"], 4), "raster_ms": round(med["raster"], 4), "prepare_ms": round(med["prepare"], 4),
               "upload_ms": round(med["upload"], 4), "upload_plus_prepare_ms": round(med["upload"] + med["prepare"], 4),
               "strokes_over_replaced": round(med["strokes"] / (med["upload"] + med["prepare"]), 3),
               "spread_ms": {k: [round(min(v), 4), round(max(v), 4)] for k, v in times.items()}}
        rows.append(row)
        print(json.dumps(row), flush=True)
    res = {"bench": "raster", "runs": a.runs, "inner": a.inner, "device": torch.cuda.get_device_name(0), "rows": rows}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return res


if __name__ == "__main__":
    main()
