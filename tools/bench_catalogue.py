"""What opening a brush picker costs: icon and clear-background factor of every brush of a 100-seed library at R = 256, default conv
mode, five calibration drawings -- one brush at a time, as before the catalogue, against ``StyleUVSMapper.catalogue(batch=32)``.

  (a) per brush   the factor by the per-brush method kept verbatim below (one generator pass of the 5 drawings, then five
                  ``torch.topk(S[i][bmask[i]], k=15)`` selections, each behind a boolean-mask gather that waits for the device), plus
                  one icon render per brush (``get_brush_icon``: a generator pass on the first drawing, the icon copied to the host);
  (b) catalogue   ``catalogue(library, batch=32)``: six brushes per generator pass, one selection launch per pass, icons, colours and
                  factors copied to the host at the end.

Both are warmed, then alternated within this process for --repeats rounds; every time is the host clock around work that ends in a
device synchronise.  The results of the last round are compared (the factors, the background weights they are the reciprocals of,
the share of icon bytes that differ), so that faster does not mean different.

    python tools/bench_catalogue.py [--repeats 5] [--brushes 100] [--out profiles/catalogue_bench.json]

The selection kernel's own time comes from a separate ``rocprofv3 --kernel-trace --stats`` run of this tool (--repeats 1).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from brushstroke_engine_amd import build, config as cfgmod, encoder as encmod, formats, painting, weights as wmod  # noqa: E402

R = 256


def calibration_drawings(r, k=5):
    """[2,k,r,r] uint8 (medium, thick), 255 = background: the synthetic stand-ins of tests/golden/make_golden_engine.py at patch size r."""
    cal = np.full((2, k, r, r), 255, np.uint8)
    for i in range(k):
        for thick, half in ((0, 3 * r // 128), (1, 6 * r // 128)):
            for t in np.linspace(0, 1, 4 * r):
                yy = int(r * (0.2 + 0.6 * t))
                xx = int(r * (0.5 + 0.3 * np.sin(t * (i + 1) * 1.7 + i)))
                cal[thick, i, max(yy - half, 0):yy + half, max(xx - half, 0):xx + half] = 0
    return cal


def sfactor_per_brush(mapper, opts):
    """``StyleUVSMapper.get_sfactor`` as it was before ``calibrate`` (without its cache)."""
    n = mapper.geom_feature[0].shape[0]
    ws = mapper.ops.map_style(z=opts.style_z, ws=opts.style_ws).expand(n, -1, -1).contiguous()
    S = mapper.ops.background_weight(ws, mapper.geom_feature)
    val = torch.stack([torch.topk(S[i][mapper.bmask[i]], k=15)[0].min() for i in range(n)]).min()
    return 1 / val


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
        raise SystemExit("bench_catalogue needs a GPU: a CPU run says nothing about kernels or copies")
    from brushstroke_engine_amd.networks import DEFAULT_CONV_MODE, Generator
    dev = torch.device("cuda:0")
    cfg = cfgmod.style1_config(R)
    mode = a.conv_mode or DEFAULT_CONV_MODE
    G = Generator(cfg, wmod.random_state_dict(cfg, seed=0), conv_mode=mode).to(dev)
    ops = painting.TileOps(G, encmod.HipGeometryEncoder(encmod.random_encoder_state_dict(5), device=dev))
    cal = calibration_drawings(R)
    mapper = painting.StyleUVSMapper(ops, cal[0], cal[1])
    library = formats.SeedBrushLibrary(list(range(a.brushes)), cfg.z_dim)
    ids = library.get_style_ids()

    def per_brush():
        sf, icons = [], []
        for sid in ids:
            opts = painting.GanBrushOptions()
            library.set_style(sid, opts)
            sf.append(sfactor_per_brush(mapper, opts))
            icons.append(mapper.get_brush_icon(opts))
        sf = torch.stack(sf)
        torch.cuda.synchronize()
        return sf.cpu().numpy(), np.stack(icons)

    def catalogue():
        mapper.sfactors = {}
        cat = mapper.catalogue(library, batch=a.batch)
        torch.cuda.synchronize()
        return cat.sfactors, cat.icons

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        return (time.perf_counter() - t0) * 1e3, out

    with torch.no_grad():
        per_brush(), catalogue()                                    # warm-up: workspaces of both batch sizes, code objects
        times = {"per_brush": [], "catalogue": []}
        for _ in range(a.repeats):
            ms, old = timed(per_brush)
            times["per_brush"].append(ms)
            ms, new = timed(catalogue)
            times["catalogue"].append(ms)
    res = {"bench": "catalogue", "device": torch.cuda.get_device_name(0), "conv_mode": mode, "resolution": R, "brushes": len(ids),
           "drawings": int(cal.shape[1]), "batch": a.batch, "repeats": a.repeats}
    for name, t in times.items():
        res[name] = {"median_ms": round(float(np.median(t)), 3), "min_ms": round(min(t), 3), "max_ms": round(max(t), 3),
                     "all_ms": [round(x, 3) for x in t]}
    spread = max(res[n]["max_ms"] - res[n]["min_ms"] for n in times)
    res["gain_ms"] = round(res["per_brush"]["median_ms"] - res["catalogue"]["median_ms"], 3)
    res["spread_ms"] = round(spread, 3)
    res["catalogue_faster_beyond_spread"] = bool(res["gain_ms"] > spread)
    # the factor is 1 / (a background weight in 0..1): where a brush's weight is small, the conv mode's absolute error on it is a large
    # relative one, so the weights themselves are compared too
    res["sfactor_median_rel_diff"] = float(np.median(np.abs(new[0] / old[0] - 1)))
    res["sfactor_max_rel_diff"] = float(np.abs(new[0] / old[0] - 1).max())
    res["background_weight_max_abs_diff"] = float(np.abs(1 / new[0] - 1 / old[0]).max())
    res["background_weight_min"] = float((1 / old[0]).min())
    res["icon_bytes_differing"] = float((new[1] != old[1]).mean())
    res["icon_max_byte_diff"] = int(np.abs(new[1].astype(np.int32) - old[1].astype(np.int32)).max())
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return res


if __name__ == "__main__":
    main()
