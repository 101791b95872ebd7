"""Preparing a drawing for the tiled schedule, host route against device route, on the same box in the same process.

  host    painting.prepare_geometry_image + pad_geo + generate_stitching_crops(mode="stroke") in numpy, then the upload of the padded
          geometry (host clock around work that ends in a device synchronise);
  device  the upload of the decoded drawing, nb_geom_prepare_u8 into the padded buffer, nb_tile_stroke_counts_u8 and the read-back of
          the per-tile counts (HIP events, and the host clock around the same work).

Synthetic drawings (random thick polylines on white) at 1024^2 and 4096^2, RGB and RGBA; the two routes alternate, medians of --runs
repetitions after a warm-up; both routes' geometry and tile lists are compared before anything is timed.  The crop + composite on
white is timed apart (kernel against the torch expression of paint_image).

    python tools/bench_prepare.py [--runs 7] [--sizes 1024,4096] [--out profiles/prepare.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from brushstroke_engine_amd import build, painting  # noqa: E402
from bench_canvas import synthetic_drawing  # noqa: E402


class PrepOps(painting.TileOps):
    """The preparation entries of TileOps without a generator behind them."""

    def __init__(self, device, patch_width):
        self.device, self.patch_width = torch.device(device), patch_width


def drawing(size, channels, seed=0):
    """Decoded drawing: dark strokes of varying gray on white (RGB), or black strokes with soft alpha on transparent (RGBA)."""
    stroke = synthetic_drawing(size, size, seed=seed)[..., 0] == 0
    rs = np.random.RandomState(seed + 1)
    if channels == 3:
        img = np.full((size, size, 3), 255, np.uint8)
        img[stroke] = rs.randint(0, 90, (int(stroke.sum()), 3))
        return img
    img = np.zeros((size, size, 4), np.uint8)
    img[stroke, 3] = rs.randint(160, 256, int(stroke.sum()))
    return img


def median(xs):
    return float(np.median(np.asarray(xs)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--sizes", default="1024,4096")
    ap.add_argument("--patch", type=int, default=256)
    ap.add_argument("--crop_margin", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    build.build(verbose=False)
    if not torch.cuda.is_available():
        raise SystemExit("bench_prepare needs a GPU: a CPU run says nothing about either route's upload or kernels")
    dev = torch.device("cuda:0")
    ops = PrepOps(dev, a.patch)
    R, m = a.patch, a.crop_margin
    rows = []
    for size in [int(s) for s in a.sizes.split(",")]:
        for channels in (3, 4):
            img = drawing(size, channels)

            def host_route():
                geom = painting.prepare_geometry_image(img)
                crops, padded = painting.generate_stitching_crops(painting.pad_geo(geom, m), R, "stroke", 2 * m)
                padded_dev = ops.to_device(padded[..., 0])
                torch.cuda.synchronize(dev)
                return crops, padded_dev

            def device_route():
                nrows, ncols, stride, ph, pw = painting.stitching_grid(size + m, size + m, R, 2 * m)
                padded_dev = ops.prepare_geometry(img, (ph, pw), (m, m))                # uploads img
                keep = ops.to_host(ops.stroke_counts(padded_dev, R, stride, nrows, ncols)) > 10      # synchronises
                return [(int(r) * stride, int(c) * stride, R, R) for r, c in zip(*np.nonzero(keep))], padded_dev

            (crops_h, pad_h), (crops_d, pad_d) = host_route(), device_route()              # warm-up of both, and the comparison
            assert crops_h == crops_d and torch.equal(pad_h, pad_d), "the two routes disagree"
            device_route()
            t_host, t_dev_ev, t_dev_wall = [], [], []
            for _ in range(a.runs):
                t0 = time.perf_counter()
                host_route()
                t_host.append((time.perf_counter() - t0) * 1e3)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                e0.record()
                device_route()
                e1.record()
                torch.cuda.synchronize(dev)
                t_dev_wall.append((time.perf_counter() - t0) * 1e3)
                t_dev_ev.append(e0.elapsed_time(e1))
            # the kernels alone (drawing already on the device): what a C host with a resident image pays
            img_dev = ops.to_device(img)
            nrows, ncols, stride, ph, pw = painting.stitching_grid(size + m, size + m, R, 2 * m)
            t_kern = []
            for _ in range(a.runs + 2):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                ops.stroke_counts(ops.prepare_geometry(img_dev, (ph, pw), (m, m)), R, stride, nrows, ncols)
                e1.record()
                torch.cuda.synchronize(dev)
                t_kern.append(e0.elapsed_time(e1))
            # crop + on-white: kernel against the torch expression of paint_image
            canvas = torch.randint(0, 256, [ph, pw, 4], dtype=torch.uint8, device=dev)

            def torch_white():
                result = canvas[m:m + size, m:m + size]
                lut = ops.to_device(np.arange(256, dtype=np.float32) / np.float32(255))
                al = lut[result[..., 3:].to(torch.int64)]
                return (result[..., :3].to(torch.float32) * al + 255 * (1 - al)).clip(0, 255).to(torch.uint8).contiguous()
            assert torch.equal(torch_white(), ops.composite_on_white(canvas, m, m, size, size))
            t_white = {"torch": [], "kernel": []}
            for _ in range(a.runs + 2):
                for name, fn in (("torch", torch_white), ("kernel", lambda: ops.composite_on_white(canvas, m, m, size, size))):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn()
                    e1.record()
                    torch.cuda.synchronize(dev)
                    t_white[name].append(e0.elapsed_time(e1))
            row = {"size": size, "channels": channels, "patch": R, "tiles_kept": len(crops_d), "tiles": nrows * ncols,
                   "host_route_ms": round(median(t_host), 3), "device_route_ms": round(median(t_dev_ev), 3),
                   "device_route_wall_ms": round(median(t_dev_wall), 3), "host_over_device": round(median(t_host) / median(t_dev_ev), 1),
                   "device_kernels_only_ms": round(median(t_kern[2:]), 4),
                   "on_white_torch_ms": round(median(t_white["torch"][2:]), 4), "on_white_kernel_ms": round(median(t_white["kernel"][2:]), 4),
                   "host_route_ms_all": [round(t, 1) for t in t_host], "device_route_ms_all": [round(t, 3) for t in t_dev_ev]}
            rows.append(row)
            print(json.dumps(row), flush=True)
    res = {"bench": "prepare", "runs": a.runs, "cpu_threads": torch.get_num_threads(), "device": torch.cuda.get_device_name(0), "rows": rows}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return res


if __name__ == "__main__":
    main()
