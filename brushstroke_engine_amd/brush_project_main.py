"""Make brushes from pictures -- the reference's ``scripts/project_main.py`` -- K exemplars per pass on the device
(``projection.BrushProjector``): W or W+ and the generator's noise planes are optimised so that the generator reproduces patches of an
exemplar image of a medium, given the drawing that goes with it.

    python -m brushstroke_engine_amd.brush_project_main --gan_checkpoint engine.npz --target_image sample.png --geom_image sample_geom.png \\
        --output_dir out [--output_style_id ID] [--target_bg_image bg.png] [--w_plus] [--no_noise] [--num_steps 1000] [--num_crops 10]
        [--patch_scale_range 0.2,0.5] [--with_positions] [--overfit_one] [--with_composite] [--l1_fg_weight X] [--bg_weight X] [--seed N]
        [--skip_existing] [--resume] [--brushes_per_pass 4] [--patches file.npz]

``--target_image`` may be repeated, each with its ``--geom_image`` (and, if any has one, its ``--target_bg_image``); the exemplars share
passes of ``--brushes_per_pass``.  ``--patches file.npz`` (``target`` [B,3,R,R] and ``geom`` [B,1,R,R] in 0..1, optionally ``positions``
[B,2] and ``target_bg``) bypasses the patch samplers; the brush is named by ``--output_style_id`` or the file.  Written into
``--output_dir``: ``ALL_projected_<suffix>.pkl`` (merged with an existing file as ``brush_clarity_main.merge_into_library`` does; what
``formats.WBrushLibrary`` reads), ``<id>_projected_<suffix>.npz`` per brush and ``projection.json`` with the loss items at the first step
and at the step a brush finished at.  ``--lpips_weights file.npz`` (written by ``tools/convert_lpips_weights.py`` from a user's weight
files; none ship) switches the reference's perceptual item on (``perceptual.LPIPS``; best state and early stop then go by its value, as
in the reference, and ``--l1_fg_weight`` / ``--bg_weight`` may both be 0); without it at least one of the two must be positive.  No
video or visualisation output.  Single process.
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

from . import projection
from .brush_clarity_main import merge_into_library

logger = logging.getLogger(__name__)


def parse_patch_range(arg_val: str):
    res = [float(x) for x in arg_val.split(",")]
    if len(res) != 2 or not (0 < res[0] <= res[1] <= 1):
        raise argparse.ArgumentTypeError(f"patch_scale_range {arg_val!r}: CSV min,max with 0 < min <= max <= 1")
    return res[0], res[1]


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="Project exemplar images of a medium into brushes on MI355X.")
    ap.add_argument("--gan_checkpoint", required=True, help=".npz engine container (generator + encoder)")
    ap.add_argument("--output_dir", required=True)
    ap.add_argument("--target_image", action="append", default=None, help="exemplar image; may be repeated")
    ap.add_argument("--geom_image", action="append", default=None, help="the drawing of each exemplar (channel 1 is read, 0 = stroke)")
    ap.add_argument("--target_bg_image", action="append", default=None, help="background image of each exemplar for --with_composite")
    ap.add_argument("--output_style_id", action="append", default=None, help="brush ids; default: the image file names")
    ap.add_argument("--patches", default=None, help=".npz with target, geom[, positions, target_bg]: bypasses the patch samplers")
    ap.add_argument("--seed", type=int, default=None)
    ap.add_argument("--w_plus", action="store_true")
    ap.add_argument("--num_steps", type=int, default=1000)
    ap.add_argument("--no_noise", action="store_true")
    ap.add_argument("--num_crops", type=int, default=10)
    ap.add_argument("--patch_scale_range", type=parse_patch_range, default=(0.2, 0.5), help="CSV min and max scale of patches, e.g. 0.2,0.5")
    ap.add_argument("--with_positions", action="store_true")
    ap.add_argument("--overfit_one", action="store_true")
    ap.add_argument("--skip_existing", action="store_true")
    ap.add_argument("--resume", action="store_true")
    ap.add_argument("--with_composite", action="store_true")
    ap.add_argument("--l1_fg_weight", type=float, default=0)
    ap.add_argument("--bg_weight", type=float, default=0)
    ap.add_argument("--brushes_per_pass", type=int, default=4, help="exemplars that share a generator batch")
    ap.add_argument("--lpips_weights", default=None, help=".npz of tools/convert_lpips_weights.py: switches the perceptual item on")
    return ap


def file_suffix(args) -> str:
    """project_main.py:539-541."""
    return ("wplus" if args.w_plus else "w") + "_" + ("fixednoise" if args.no_noise else "optnoise") + f"_ncrop{args.num_crops}"


def _read_image(fname: str) -> np.ndarray:
    from PIL import Image
    a = np.array(Image.open(fname))
    return a if a.ndim == 3 else np.repeat(a[..., None], 3, axis=2)


def load_exemplars(args, width: int) -> Dict:
    """{id: (target, geom, positions, target_bg)} from ``--patches`` or from the images through the samplers (project_main.py:574-584)."""
    if args.patches is not None:
        sid = args.output_style_id[0] if args.output_style_id else os.path.splitext(os.path.basename(args.patches))[0]
        with np.load(args.patches) as z:
            get = lambda k: torch.from_numpy(np.asarray(z[k], np.float32)) if k in z.files else None
            return {sid: (get("target"), get("geom"), get("positions"), get("target_bg"))}
    targets, geoms, bgs = args.target_image or [], args.geom_image or [], args.target_bg_image or []
    if not targets or len(geoms) != len(targets) or (bgs and len(bgs) != len(targets)):
        raise ValueError("every --target_image needs its --geom_image (and, if any is given, its --target_bg_image)")
    ids = args.output_style_id or [".".join(os.path.basename(t).split(".")[:-1]) for t in targets]
    if len(ids) != len(targets) or len(set(ids)) != len(ids):
        raise ValueError("one distinct --output_style_id per --target_image")
    out = {}
    for i, sid in enumerate(ids):
        rng = np.random.default_rng(None if args.seed is None else [args.seed, i])
        if bgs:
            tp, bp, gp, pos = projection.load_target_sparse(_read_image(targets[i]), _read_image(bgs[i]), _read_image(geoms[i]), width,
                                                            crop_n=args.num_crops, patch_range=args.patch_scale_range, rng=rng)
        else:
            tp, gp, pos = projection.load_target(_read_image(targets[i]), _read_image(geoms[i]), width, crop_n=args.num_crops,
                                                 patch_range=args.patch_scale_range, rng=rng, overfit_one=args.overfit_one)
            bp = None
        out[sid] = (tp, gp, pos, bp)
    return out


def write_records(output_dir: str, suffix: str, result: Dict, history: Dict) -> str:
    """``<id>_projected_<suffix>.npz`` per brush (project_main.py:469-470) and ``projection.json``; returns the latter's path."""
    os.makedirs(output_dir, exist_ok=True)
    info = {}
    for sid, entry in result.items():
        np.savez(os.path.join(output_dir, f"{sid}_projected_{suffix}.npz"), w=entry["w"].numpy(), bg=entry["bg"].numpy(), step=np.int64(entry["step"]),
                 **{k: v.numpy() for k, v in entry["noise"].items()})
        info[str(sid)] = {**history.get(sid, {}), "step": int(entry["step"]), "bg": [float(x) for x in entry["bg"]]}
    path = os.path.join(output_dir, "projection.json")
    with open(path, "w") as f:
        json.dump(info, f, indent=1, sort_keys=True)
    return path


def main(argv=None, engine=None):
    """``engine`` = (gen, encode, device): a generator and an encoder to use instead of ``--gan_checkpoint``'s (CPU runs, tests)."""
    args = build_parser().parse_args(argv)
    suffix = file_suffix(args)
    all_pkl = os.path.join(args.output_dir, f"ALL_projected_{suffix}.pkl")
    if engine is None:
        from . import encoder, formats, launch
        from .training import TrainableGenerator
        _, _, device, _ = launch.init()              # kernel library first, then the device
        cfg, gen_sd, enc_sd, preproc, _ = formats.load_engine_snapshot(args.gan_checkpoint)
        if not encoder.HipGeometryEncoder.supports(cfg.img_resolution):
            raise RuntimeError(f"the geometry-encoder kernels tile patches of 32, 64 or 128 k pixels; this checkpoint paints {cfg.img_resolution}")
        gen, encode = TrainableGenerator(cfg, gen_sd, device), encoder.HipGeometryEncoder(enc_sd, preproc_type=preproc, device=device).encode
    else:
        gen, encode, device = engine
    os.makedirs(args.output_dir, exist_ok=True)
    exemplars = load_exemplars(args, gen.cfg.img_resolution)
    existing = {}
    if os.path.isfile(all_pkl) and (args.skip_existing or args.resume):             # project_main.py:550-562
        with open(all_pkl, "rb") as f:
            existing = pickle.load(f)
    if args.skip_existing:
        for sid in [s for s in exemplars if s in existing]:
            logger.info(f"All pickle already has projection for {sid}, skipping: {all_pkl}")
            del exemplars[sid]
    if args.resume:
        for sid in [s for s in exemplars if s not in existing]:
            logger.info(f"cannot resume {sid}, skipping: {all_pkl}")
            del exemplars[sid]
    if not exemplars:
        return all_pkl, None
    if args.seed is not None:
        torch.manual_seed(args.seed)
    lpips = None
    if args.lpips_weights is not None:                                     # project_main.py:158: the item the reference optimises first of all
        from .perceptual import LPIPS
        lpips = LPIPS(args.lpips_weights, device=device)
    proj = projection.BrushProjector(gen, encode, device=device, perceptual=lpips, num_steps=args.num_steps, w_plus=args.w_plus, optimize_noise=not args.no_noise,
                                     with_positions=args.with_positions, with_composite=args.with_composite, l1_fg_weight=args.l1_fg_weight,
                                     bg_weight=args.bg_weight, resume_from=existing if args.resume else None)
    result = proj.project(exemplars, brushes_per_pass=args.brushes_per_pass, seed=args.seed)
    merge_into_library(all_pkl, result)
    info = write_records(args.output_dir, suffix, result, proj.history)
    for p in (all_pkl, info):
        print(p)
    return all_pkl, info


if __name__ == "__main__":
    main()
