"""Scores of a brush library -- LAB_E%, LAB_L2, BG_CLARITY_MEAN and FG_OPACITY_MEDIAN per brush, the numbers the reference's
``paint_engine_metric_loop`` reports (forger/metrics/metric_main.py:105-236) -- computed in batches on the device
(``metrics.BrushEvaluator``).  With ``--lpips_weights`` the three perceptual numbers LPIPS_ACROSS_GEO, LPIPS_UNIFORM_BG and
LPIPS_UNIFORM_BG_multicolor join them, and the files carry seven columns; with ``--stitch_drawings`` too, STITCH_L1 and STITCH_LPIPS
(two positioned renders of overlapping crops of full-size drawings, each composited into the other) make it the reference's nine.

    python -m brushstroke_engine_amd.brush_metrics_main --gan_checkpoint engine.npz --library rand100 --drawings drawings.npz \\
        --output_dir out [--uvs_calibration cal.npz] [--rounds 1] [--batch 32] [--seed 0] [--lab_thresh 10] [--prefix ''] [--conv_mode h3] \\
        [--lpips_weights alex.npz] [--lpips_net alex] [--patch_width P] \\
        [--stitch_drawings full.npz] [--stitch_margin 10] [--stitch_min_overlap 50]

``--drawings`` is an .npz whose first array (or the one named ``drawings``) holds [K,R,R] uint8 guidance drawings, 0 = stroke.
``--stitch_drawings`` is such an .npz with [Ks,D,D] full-size drawings, D above R; it needs ``--lpips_weights``.
``--library`` is what ``paint_image_main`` takes.  Three files are written to ``--output_dir``: ``<prefix>style_metrics.txt`` and
``<prefix>summary_metrics.txt`` in the reference's line format, and ``<prefix>brush_metrics.json``.  Single process.
"""
from __future__ import annotations

import argparse
import logging
import os

import numpy as np
import torch

from . import encoder, formats, launch, metrics, painting
from .networks import DEFAULT_CONV_MODE, Generator

logger = logging.getLogger(__name__)


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="Colour and transparency scores of a brush library on MI355X.")
    ap.add_argument("--gan_checkpoint", required=True, help=".npz engine container (generator + encoder)")
    ap.add_argument("--library", default="rand100")
    ap.add_argument("--drawings", required=True, help=".npz with [K,R,R] uint8 guidance drawings (0 = stroke), or synth:K[:seed[:key=value,...]] (drawings.parse_synth)")
    ap.add_argument("--uvs_calibration", default=None, help=".npz with 'medium' and 'thick' calibration drawings, or synth[:seed]: render with the brushes' factors")
    ap.add_argument("--output_dir", required=True)
    ap.add_argument("--prefix", default="", help="prefix of the three file names")
    ap.add_argument("--rounds", type=int, default=1, help="renders per brush, each with fresh primary colours")
    ap.add_argument("--batch", type=int, default=32, help="samples per generator pass: floor(batch / K) brushes on every drawing")
    ap.add_argument("--seed", type=int, default=0, help="seed of the colour stream")
    ap.add_argument("--lab_thresh", type=float, default=10)
    ap.add_argument("--conv_mode", default=None, choices=["f8", "h3", "f32"],
                    help="arithmetic of the conv layers (default: networks.DEFAULT_CONV_MODE)")
    ap.add_argument("--lpips_weights", default=None,
                    help=".npz written by tools/convert_lpips_weights.py: also report LPIPS_ACROSS_GEO, LPIPS_UNIFORM_BG and "
                         "LPIPS_UNIFORM_BG_multicolor (the reference scores with the 'alex' network)")
    ap.add_argument("--lpips_net", default=None, choices=["alex", "vgg"], help="the network of --lpips_weights (default: the file's 'arch' entry)")
    ap.add_argument("--patch_width", type=int, default=None,
                    help="side of the windows of the LPIPS_UNIFORM_BG scores (default: R / 4, R / 2 or 0.8 R, the first of at least 64)")
    ap.add_argument("--stitch_drawings", default=None,
                    help=".npz with [Ks,D,D] uint8 full-size drawings (0 = stroke), D above the patch width, or synth:Ks:seed:size=D: also report STITCH_L1 and "
                         "STITCH_LPIPS (needs --lpips_weights)")
    ap.add_argument("--stitch_margin", type=int, default=10, help="the stitcher's crop margin (RandomStitcher.crop_margin)")
    ap.add_argument("--stitch_min_overlap", type=int, default=50, help="the stitcher's minimum overlap of the two crops")
    return ap


def load_drawings(path: str, r=None, device="cpu") -> np.ndarray:
    """[K,D,D] uint8 drawings: the .npz at ``path``, or ``synth:K[:seed[:key=value,...]]`` of patch width ``r`` made on ``device``
    (``drawings.load_drawings``)."""
    from .drawings import load_drawings as load
    return load(path, r, device)


def write_scores(scores: metrics.BrushScores, out_dir: str, prefix: str = ""):
    """The two text files of ``BrushScores.write_reference_files`` and ``<prefix>brush_metrics.json``; returns the three paths."""
    style, summary = scores.write_reference_files(out_dir, prefix)
    info = os.path.join(out_dir, f"{prefix}brush_metrics.json")
    with open(info, "w") as f:
        f.write(scores.to_json())
    return style, summary, info


def main(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    if args.stitch_drawings and not args.lpips_weights:
        ap.error("--stitch_drawings needs --lpips_weights")
    _, _, device, _ = launch.init()                  # kernel library first, then the device
    cfg, gen_sd, enc_sd, preproc, _ = formats.load_engine_snapshot(args.gan_checkpoint)
    G = Generator(cfg, gen_sd, conv_mode=args.conv_mode or DEFAULT_CONV_MODE).to(device)
    if not encoder.HipGeometryEncoder.supports(cfg.img_resolution):
        raise RuntimeError(f"the geometry-encoder kernels tile patches of 32, 64 or 128 k pixels; this checkpoint paints {cfg.img_resolution}")
    ops = painting.TileOps(G, encoder.HipGeometryEncoder(enc_sd, preproc_type=preproc, device=device))
    mapper = None
    if args.uvs_calibration:
        from .drawings import load_calibration
        mapper = painting.StyleUVSMapper(ops, *load_calibration(args.uvs_calibration, cfg.img_resolution, device))
    library = formats.BrushLibrary.from_arg(args.library, z_dim=G.z_dim)
    with torch.no_grad():
        evaluator = metrics.BrushEvaluator(ops, load_drawings(args.drawings, cfg.img_resolution, device), seed=args.seed, uvs_mapper=mapper)
        kw = {}
        if args.lpips_weights:
            from .perceptual import LPIPS
            kw = dict(lpips=LPIPS(args.lpips_weights, net=args.lpips_net, device=device), patch_width=args.patch_width)
        if args.stitch_drawings:
            kw["stitch"] = metrics.StitchSetup(load_drawings(args.stitch_drawings, cfg.img_resolution, device), args.stitch_margin, args.stitch_min_overlap)
        scores = evaluator.evaluate(library, rounds=args.rounds, batch=args.batch, lab_thresh=args.lab_thresh, **kw)
    paths = write_scores(scores, args.output_dir, args.prefix)
    logger.info(f"Scored {len(scores.ids)} brushes: {paths}")
    for p in paths:
        print(p)
    return paths


if __name__ == "__main__":
    main()
