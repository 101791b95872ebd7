"""Clarity optimisation of a brush library -- the reference's ``scripts/opt_clarity_main.py`` -- in batches on the device
(``clarity.ClarityOptimizer``): brushes whose background is not clear are optimised in W+ and in the generator's noise planes, and
written into a W library that ``paint_image_main`` / ``brush_metrics_main`` / ``formats.WBrushLibrary`` read.

    python -m brushstroke_engine_amd.brush_clarity_main --gan_checkpoint engine.npz --library rand100 --drawings drawings.npz \\
        --out_library default --output_dir out [--brush_id ID] [--batch_size 20] [--num_steps 1000] [--losses STRING] [--seed N]
        [--brushes_per_pass 4] [--uvs_calibration cal.npz] [--lpips_weights lpips_vgg.npz]

``--lpips_weights`` (the file ``tools/convert_lpips_weights.py`` writes; no weights ship) loads ``perceptual.LPIPS`` and allows
``lpips(<component>)`` in ``--losses``, e.g. the reference's default ``0.5*iou_inv(uvs)+0.5*iou(u)+50*lpips(fake_orig)+50*l1(fake_orig)``;
the default string here stays without the item.

``--drawings`` is the .npz of ``brush_metrics_main.load_drawings`` ([K,R,R] uint8, 0 = stroke): the conditioning and the truth of the
loss, and the drawings the before / after scores are taken on.  ``--out_library default`` writes ``OPT_<library name>`` beside the
library (into ``--output_dir`` when the library is not a file).  Written: the pickle W library (merged with an existing file; an entry
that is already there is overwritten with a warning, opt_clarity_main.py:255-265), ``<id>_opt_optimized.npz`` per brush, and
``clarity.json``: per brush the loss items at the first and the last step and BG_CLARITY_MEAN / FG_OPACITY_MEDIAN before and after
(``metrics.BrushEvaluator``).  Single process.
"""
from __future__ import annotations

import argparse
import json
import logging
import os
import pickle
from typing import Dict

import numpy as np
import torch

from . import clarity

logger = logging.getLogger(__name__)


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="Optimise brushes of a library for a clear background on MI355X.")
    ap.add_argument("--gan_checkpoint", required=True, help=".npz engine container (generator + encoder)")
    ap.add_argument("--library", required=True, help="what paint_image_main takes: a file, rand<N>, a seed count or a seed list")
    ap.add_argument("--drawings", required=True, help=".npz with [K,R,R] uint8 guidance drawings (0 = stroke), or synth:K[:seed[:key=value,...]]")
    ap.add_argument("--out_library", required=True, help='output W library (pickle), or "default"')
    ap.add_argument("--output_dir", required=True)
    ap.add_argument("--brush_id", default=None, help="optimise this brush only (default: the whole library)")
    ap.add_argument("--batch_size", type=int, default=20, help="drawings per step")
    ap.add_argument("--num_steps", type=int, default=1000)
    ap.add_argument("--losses", default=clarity.DEFAULT_LOSSES)
    ap.add_argument("--seed", type=int, default=None)
    ap.add_argument("--brushes_per_pass", type=int, default=4, help="brushes that share an encoder pass and a generator batch")
    ap.add_argument("--uvs_calibration", default=None, help=".npz with 'medium' and 'thick' calibration drawings, or synth[:seed]: score with the brushes' factors")
    ap.add_argument("--lpips_weights", default=None, help=".npz of tools/convert_lpips_weights.py: allows lpips(<component>) in --losses")
    return ap


def default_out_library(library: str, output_dir: str) -> str:
    """``OPT_<name>`` beside a library file (opt_clarity_main.py:307-309); for ``rand<N>`` or a seed list, in the output directory."""
    if os.path.isfile(library):
        return os.path.join(os.path.dirname(library), "OPT_" + os.path.basename(library))
    return os.path.join(output_dir, "OPT_" + library.replace(",", "_") + ".pkl")


def merge_into_library(path: str, entries: Dict) -> Dict:
    """opt_clarity_main.py:255-265: load the pickle if it is there, overwrite entries that exist (with a warning), write it back."""
    all_data = {}
    if os.path.isfile(path):
        with open(path, "rb") as f:
            all_data = pickle.load(f)
    for bid, entry in entries.items():
        if bid in all_data:
            logger.warning(f"All pickle already has projection for {bid}, overwriting entry in: {path}")
        all_data[bid] = entry
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "wb") as f:
        pickle.dump(all_data, f)
    return all_data


def write_records(output_dir: str, result: Dict, history: Dict, before=None, after=None) -> str:
    """``<id>_opt_optimized.npz`` per brush (w and the noise planes) and ``clarity.json``; returns the latter's path."""
    os.makedirs(output_dir, exist_ok=True)
    info = {}
    for i, (bid, entry) in enumerate(result.items()):
        np.savez(os.path.join(output_dir, f"{bid}_opt_optimized.npz"), w=entry["w"].numpy(), **{k: v.numpy() for k, v in entry["noise"].items()})
        info[str(bid)] = dict(history.get(bid, {}))
        for key, scores in (("before", before), ("after", after)):
            if scores is not None:
                info[str(bid)][key] = {"BG_CLARITY_MEAN": float(scores.bg_clarity_mean[i]), "FG_OPACITY_MEDIAN": float(scores.fg_opacity_median[i])}
    path = os.path.join(output_dir, "clarity.json")
    with open(path, "w") as f:
        json.dump(info, f, indent=1, sort_keys=True)
    return path


def main(argv=None):
    args = build_parser().parse_args(argv)
    from . import encoder, formats, launch, metrics, painting
    from .brush_metrics_main import load_drawings
    from .networks import Generator
    from .training import TrainableGenerator
    _, _, device, _ = launch.init()                  # kernel library first, then the device
    cfg, gen_sd, enc_sd, preproc, _ = formats.load_engine_snapshot(args.gan_checkpoint)
    if not encoder.HipGeometryEncoder.supports(cfg.img_resolution):
        raise RuntimeError(f"the geometry-encoder kernels tile patches of 32, 64 or 128 k pixels; this checkpoint paints {cfg.img_resolution}")
    enc = encoder.HipGeometryEncoder(enc_sd, preproc_type=preproc, device=device)
    drawings = load_drawings(args.drawings, cfg.img_resolution, device)
    library = formats.BrushLibrary.from_arg(args.library, z_dim=cfg.z_dim)
    ids = [args.brush_id] if args.brush_id is not None else list(library.get_style_ids())
    out_library = default_out_library(args.library, args.output_dir) if args.out_library == "default" else args.out_library
    logger.info(f"Writing out to library: {out_library}")
    os.makedirs(args.output_dir, exist_ok=True)

    ops = painting.TileOps(Generator(cfg, gen_sd).to(device), enc)
    mapper = None
    if args.uvs_calibration:
        from .drawings import load_calibration
        mapper = painting.StyleUVSMapper(ops, *load_calibration(args.uvs_calibration, cfg.img_resolution, device))
    with torch.no_grad():
        evaluator = metrics.BrushEvaluator(ops, drawings, seed=args.seed or 0, uvs_mapper=mapper)
        before = evaluator.evaluate(library, style_ids=ids)
    lpips = None
    if args.lpips_weights is not None:
        from .perceptual import LPIPS
        lpips = LPIPS(args.lpips_weights, device=device)
    opt = clarity.ClarityOptimizer(TrainableGenerator(cfg, gen_sd, device), enc.encode, drawings, losses=args.losses, lpips=lpips)
    result = opt.optimize(library, style_ids=ids, num_steps=args.num_steps, batch_size=args.batch_size, brushes_per_pass=args.brushes_per_pass,
                          seed=args.seed)
    with torch.no_grad():
        after = evaluator.evaluate(formats.WBrushLibrary(result), style_ids=ids)
    merge_into_library(out_library, result)
    info = write_records(args.output_dir, result, opt.history, before, after)
    for p in (out_library, info):
        print(p)
    return out_library, info


if __name__ == "__main__":
    main()
