"""The paint session against the paths it is meant to spare, on the same box in the same process: a 4096^2 drawing at R = 256.

  add            PaintSession.add of strokes that touch 1, 4 and 16 tiles (each followed by an undo outside the timed window);
  paint_strokes  PaintingHelper.paint_strokes of the whole drawing (every tile of the grid), what one more stroke costs without a session;
  render_stroke  PaintingHelper.render_stroke of one loose tile (hipGraph replay of the generator passes);
  over_tiles     nb_over_tiles_u8 alone, all tiles of the grid over the canvas: tiles of random bytes (every alpha pair, the full
                 arithmetic at every pixel), and tiles shaped like strokes (a band of opaque pixels with soft edges on transparent ground);
  view           nb_canvas_view_u8 of the whole drawing at k = 1, 4 and 16, RGBA and on white;
  copy           a device-to-device copy of a buffer of the canvas' size: the box's copy rate, beside which the two kernels are read.

HIP events on the caller's stream around each call (an add synchronises inside -- it reads the tile picks back -- so its events span
the host's share too); medians of --runs after a warm-up; the kernels in windows of --inner back-to-back launches.  Bytes are what the
algorithm needs: 12 per covered canvas pixel for the over (source, destination, result), the window plus the output for the view.

    python tools/bench_session.py [--runs 9] [--inner 10] [--out profiles/session_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from brushstroke_engine_amd import build, config as cfgmod, encoder as encmod, painting, weights as wmod  # noqa: E402

SIZE, R, M = 4096, 256, 10


def block_strokes(row, col, n, stride):
    """Strokes that touch exactly the n x n tiles from (row, col): one horizontal line per tile row, inside the band of drawing rows
    that only that tile row's windows hold, from the first column's own band to the last one's."""
    own0, own1 = R - stride, stride                       # [own0, own1) of a window belongs to no neighbour
    s = painting.StrokeList()
    for i in range(n):
        y = (row + i) * stride + (own0 + own1) // 2 - M
        s.add_polyline([[col * stride + own0 + 12 - M, y], [(col + n - 1) * stride + own1 - 12 - M, y + 9.5]], 4.0)
    return s


def whole_drawing_strokes(seed=0, n=160):
    rs = np.random.RandomState(seed)
    s = painting.StrokeList()
    for _ in range(n):
        p = rs.uniform(0, SIZE, (1, 2)) + np.cumsum(rs.uniform(-90, 90, (8, 2)), axis=0)
        s.add_spline(p, float(rs.uniform(2, 5)))
    return s


def timed(fn, after=None):
    """(HIP-event ms, wall ms) of one call."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    if after is not None:
        after()
    return e0.elapsed_time(e1), wall


def window(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / inner


def p50(pairs):
    return {"ms": round(float(np.median([p[0] for p in pairs])), 4), "wall_ms": round(float(np.median([p[1] for p in pairs])), 4),
            "spread_ms": [round(min(p[0] for p in pairs), 4), round(max(p[0] for p in pairs), 4)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--conv-mode", default="f8")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    build.build(verbose=False)
    if not torch.cuda.is_available():
        raise SystemExit("bench_session needs a GPU: a CPU run says nothing about kernels or copies")
    from brushstroke_engine_amd.networks import Generator
    dev = torch.device("cuda:0")
    cfg = cfgmod.style1_config(R)
    G = Generator(cfg, wmod.random_state_dict(cfg, seed=0), conv_mode=a.conv_mode).to(dev)
    ops = painting.TileOps(G, encmod.HipGeometryEncoder(encmod.random_encoder_state_dict(5), device=dev))
    opts = painting.GanBrushOptions()
    opts.set_style(torch.from_numpy(np.random.RandomState(594).randn(1, cfg.z_dim)), 594)
    nrows, ncols, stride, ph, pw = painting.stitching_grid(SIZE + M, SIZE + M, R, 2 * M)
    res = {"bench": "session", "runs": a.runs, "inner": a.inner, "device": torch.cuda.get_device_name(0), "conv_mode": a.conv_mode,
           "drawing": [SIZE, SIZE], "canvas": [ph, pw], "grid": [nrows, ncols], "tile": R, "levels": {}}
    everything = whole_drawing_strokes()
    with torch.no_grad():
        for level in (0, 2):
            helper = painting.PaintingHelper(ops, batch=32)
            helper.set_feature_blending(level)
            session = painting.PaintSession(helper, (SIZE, SIZE), crop_margin=M)
            row = {}
            for n in (1, 2, 4):
                strokes = block_strokes(7, 7, n, stride)
                for _ in range(3):                                         # warm-up: workspaces of this batch size, code objects
                    session.add(strokes, opts)
                    assert session.last_tiles == n * n, (session.last_tiles, n)
                    session.undo()
                row[f"add_{n * n}_tiles"] = p50([timed(lambda: session.add(strokes, opts), session.undo) for _ in range(a.runs)])
            whole = painting.PaintingHelper(ops, batch=32)
            whole.set_feature_blending(level)
            paint = lambda: whole.paint_strokes(everything, (SIZE, SIZE), opts, crop_margin=M)     # noqa: E731
            paint()
            row["paint_strokes_whole"] = p50([timed(paint) for _ in range(max(3, a.runs // 3))])
            loose = painting.PaintingHelper(ops, batch=32)
            loose.make_new_canvas(ph, pw, level)
            patch = np.zeros((R, R, 1), np.uint8)
            patch[100:110, 40:200] = 255
            meta = {"x": 7 * stride, "y": 7 * stride, "crop_margin": M}
            tile = lambda: loose.render_stroke(patch, None, opts, meta)                            # noqa: E731
            for _ in range(3):
                tile()
            row["render_stroke"] = p50([timed(tile) for _ in range(a.runs)])
            row["add_1_below_paint_strokes"] = row["add_1_tiles"]["ms"] < row["paint_strokes_whole"]["ms"]
            res["levels"][str(level)] = row
            print(json.dumps({"level": level, **row}), flush=True)
            del session, helper, whole, loose
    # the two kernels alone, beside the box's copy rate
    canvas = torch.zeros([ph, pw, 4], dtype=torch.uint8, device=dev)
    spare = torch.empty_like(canvas)
    yx = np.stack(np.meshgrid(np.arange(nrows) * stride, np.arange(ncols) * stride, indexing="ij"), axis=-1).reshape(-1, 2)
    tiles = torch.randint(0, 256, [yx.shape[0], R, R, 4], dtype=torch.uint8, device=dev)
    rects = np.concatenate([yx + M, yx + R - M], axis=1)
    off, lst = painting.build_cells(rects, ph, pw)
    d_yx, d_off, d_lst = ops.to_device(yx.astype(np.int32)), ops.to_device(off), ops.to_device(lst)
    covered = np.zeros((ph, pw), bool)
    for y0, x0, y1, x1 in rects.tolist():
        covered[y0:y1, x0:x1] = True
    stroke_like = tiles.clone()
    ramp = torch.tensor([0, 64, 128, 191], dtype=torch.uint8, device=dev)
    alpha = torch.zeros([R], dtype=torch.uint8, device=dev)
    alpha[80:176] = 255
    alpha[76:80], alpha[176:180] = ramp, ramp.flip(0)
    stroke_like[..., 3] = alpha[None, :, None]
    fns = {"copy": (lambda: spare.copy_(canvas), 2 * canvas.numel()),
           "over_tiles_paint_stroke_like": (lambda: ops.over_tiles(canvas, stroke_like, d_yx, M, d_off, d_lst, None, 0, 255), 12 * int(covered.sum())),
           "over_tiles_paint": (lambda: ops.over_tiles(canvas, tiles, d_yx, M, d_off, d_lst, None, 0, 255), 12 * int(covered.sum())),
           "over_tiles_erase": (lambda: ops.over_tiles(canvas, tiles, d_yx, M, d_off, d_lst, None, 1, 128), 12 * int(covered.sum()))}
    for k in (1, 4, 16):
        for on_white in (False, True):
            out_bytes = (-(-SIZE // k)) ** 2 * (3 if on_white else 4)
            fns[f"view_k{k}{'_on_white' if on_white else ''}"] = (
                lambda k=k, w=on_white: ops.canvas_view(canvas, M, M, SIZE, SIZE, k, w), SIZE * SIZE * 4 + out_bytes)
    times = {name: [] for name in fns}
    for name, (fn, _) in fns.items():
        window(fn, 2)
    for _ in range(a.runs):
        for name, (fn, _) in fns.items():
            times[name].append(window(fn, a.inner))
    res["kernels"] = {}
    for name, (_, nbytes) in fns.items():
        ms = float(np.median(times[name]))
        res["kernels"][name] = {"ms": round(ms, 4), "bytes": nbytes, "gb_per_s": round(nbytes / ms / 1e6, 1),
                                "spread_ms": [round(min(times[name]), 4), round(max(times[name]), 4)]}
    res["kernels"]["tiles"] = int(yx.shape[0])
    print(json.dumps(res["kernels"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return res


if __name__ == "__main__":
    main()
