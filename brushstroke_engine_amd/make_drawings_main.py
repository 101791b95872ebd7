"""Synthetic stroke drawings into an .npz (and PNGs): ``scripts/create_splines.py`` of the reference, seeded and on the device.

    python -m brushstroke_engine_amd.make_drawings_main --samples 8 --width 256 --out drawings.npz [--seed 0] [--smart_sampling] \\
        [--pts_min 4] [--pts_max 15] [--thick_dist gauss|rand] [--centers 6,10] [--sigmas 2,3] [--prob 6,10] [--min_thickness 1] \\
        [--max_thickness 30] [--use_radii 16 25] [--png_dir DIR] [--offset 0] [--device cuda|cpu]

The flags the reference has keep its names and defaults (create_splines.py:68-77, spline_dist.py:60-67 and 90-93).  Thickness numbers
are taken as the reference states them, for 256-pixel patches, and scaled by ``width / 256``; ``--use_radii`` are pixels as given.  The
.npz holds ``drawings`` [K,R,R] uint8 (0 = stroke) -- what ``--drawings`` of the brush tools reads --, ``radii`` [K] and the flags;
``--use_radii`` with several radii draws every curve at each of them (``drawings`` radius-major per curve, as the reference's file
names sort), and with exactly two also writes ``medium`` / ``thick``: the file ``--uvs_calibration`` reads.  PNGs are named
``spline%06d_rad%03d.png``.  Without a GPU (``--device cpu``) the float64 restatements draw."""
from __future__ import annotations

import argparse
import logging
import os

import numpy as np
import torch

from . import drawings as dr

logger = logging.getLogger(__name__)


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="Seeded random spline drawings, rasterised in batches on MI355X.")
    ap.add_argument("--samples", type=int, required=True, help="number of curves")
    ap.add_argument("--width", type=int, default=256, help="side of the square drawings")
    ap.add_argument("--out", required=True, help=".npz to write")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--offset", type=int, default=0, help="number of the first curve (curve i of a seed is the same in every run)")
    ap.add_argument("--smart_sampling", action="store_true", help="control points in distinct cells of a 4 x 4 grid")
    ap.add_argument("--pts_min", type=int, default=4)
    ap.add_argument("--pts_max", type=int, default=15)
    ap.add_argument("--thick_dist", default="gauss", choices=["gauss", "rand"])
    ap.add_argument("--centers", default="6.0,10.0", help="comma-separated Gaussian centres (for 256-pixel patches)")
    ap.add_argument("--sigmas", default="2.0,3.0")
    ap.add_argument("--prob", default="6.0,10.0", help="comma-separated weights; need not be normalised")
    ap.add_argument("--min_thickness", type=int, default=1)
    ap.add_argument("--max_thickness", type=int, default=30)
    ap.add_argument("--use_radii", nargs="+", type=int, default=None, help="the same radii (pixels) for every curve, no thickness sampling")
    ap.add_argument("--png_dir", default=None, help="also write spline%%06d_rad%%03d.png files there")
    ap.add_argument("--device", default=None, help="cuda (default when there is one) or cpu")
    return ap


def spec_from_args(args) -> dr.SplineSpec:
    floats = lambda text: tuple(float(v) for v in text.split(","))          # noqa: E731
    return dr.SplineSpec(pts_min=args.pts_min, pts_max=args.pts_max, mode="cells" if args.smart_sampling else "uniform",
                         thick="mixture" if args.thick_dist == "gauss" else "range", rmin=args.min_thickness, rmax=args.max_thickness,
                         centers=floats(args.centers), sigmas=floats(args.sigmas), weights=floats(args.prob)).scaled(args.width)


def main(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    if args.samples < 1:
        ap.error("--samples must be at least 1")
    try:
        spec = spec_from_args(args)
    except ValueError as e:
        ap.error(str(e))
    device = args.device or ("cuda" if torch.cuda.is_available() else "cpu")
    synth = dr.SplineSynth(spec, args.width, args.seed, device)
    k = args.samples
    out = {"width": args.width, "seed": args.seed, "offset": args.offset, "mode": spec.mode}
    if args.use_radii:
        sets = [synth.batch(k, args.offset, spec.fixed(rad)).cpu().numpy() for rad in args.use_radii]
        out["drawings"] = np.stack(sets, axis=1).reshape(-1, args.width, args.width)
        radii = np.tile(np.asarray(args.use_radii, np.int32), k)
        if len(sets) == 2:
            out["medium"], out["thick"] = sets
    else:
        out["drawings"] = synth.batch(k, args.offset).cpu().numpy()
        radii = dr.synth_radii_numpy(spec, args.seed, args.offset, k).astype(np.int32)
    out["radii"] = radii
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    np.savez_compressed(args.out, **out)
    logger.info(f"Saved {out['drawings'].shape[0]} drawings to: {args.out}")
    print(args.out)
    if args.png_dir:
        per = len(args.use_radii) if args.use_radii else 1
        dr.save_pngs(args.png_dir, out["drawings"], lambda i: radii[i], per=per, first=args.offset)
        print(args.png_dir)
    return args.out


if __name__ == "__main__":
    main()
