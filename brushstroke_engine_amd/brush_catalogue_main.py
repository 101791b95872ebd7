"""What a brush picker shows for a brush library -- an icon, the three colours and the clear-background factor of every brush --
computed in batches on the device (``painting.StyleUVSMapper.catalogue``; the reference renders them one brush at a time for its
``brushinfo`` request, ``forger/ui/util.py:129-134``).

    python -m brushstroke_engine_amd.brush_catalogue_main --gan_checkpoint engine.npz --library rand100 \\
        --uvs_calibration cal.npz --output_file_prefix out/lib [--icon_k 4] [--cols 10] [--batch 32] [--conv_mode h3]

``--library`` is what ``paint_image_main`` takes: ``rand<N>``, a library file, a seed count or a comma separated seed list.  Two files are
written: ``<prefix>_sheet.png``, the icons side by side (``--cols`` per row, each reduced by ``--icon_k`` on the device), and
``<prefix>.json`` with the ids, the colour specs ('rgb(r,g,b):rgb(r,g,b):rgb(r,g,b)') and the factors.  Single process.
"""
from __future__ import annotations

import argparse
import logging
import os

import numpy as np
import torch

from . import encoder, formats, painting
from . import launch
from .networks import DEFAULT_CONV_MODE, Generator

logger = logging.getLogger(__name__)


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="Icons, colours and clear-background factors of a brush library on MI355X.")
    ap.add_argument("--gan_checkpoint", required=True, help=".npz engine container (generator + encoder)")
    ap.add_argument("--library", default="rand100")
    ap.add_argument("--uvs_calibration", required=True, help=".npz with 'medium' and 'thick' [5,R,R] uint8 calibration drawings, or synth[:seed]")
    ap.add_argument("--output_file_prefix", required=True)
    ap.add_argument("--icon_k", type=int, default=1, help="reduce the icons by this factor (1..16, a divisor of the patch width)")
    ap.add_argument("--cols", type=int, default=10, help="icons per row of the contact sheet")
    ap.add_argument("--batch", type=int, default=painting.StyleUVSMapper.DEFAULT_BATCH,
                    help="samples per generator pass: floor(batch / drawings) brushes on every calibration drawing")
    ap.add_argument("--conv_mode", default=None, choices=["f8", "h3", "f32"],
                    help="arithmetic of the conv layers (default: networks.DEFAULT_CONV_MODE)")
    return ap


def write_catalogue(cat: painting.BrushCatalogue, prefix: str, cols: int):
    """``<prefix>_sheet.png`` and ``<prefix>.json``; returns both paths."""
    os.makedirs(os.path.dirname(os.path.abspath(prefix)), exist_ok=True)
    sheet = cat.save_sheet(prefix + "_sheet.png", cols)
    with open(prefix + ".json", "w") as f:
        f.write(cat.to_json())
    return sheet, prefix + ".json"


def main(argv=None):
    args = build_parser().parse_args(argv)
    _, _, device, _ = launch.init()                  # kernel library first, then the device
    cfg, gen_sd, enc_sd, preproc, _ = formats.load_engine_snapshot(args.gan_checkpoint)
    G = Generator(cfg, gen_sd, conv_mode=args.conv_mode or DEFAULT_CONV_MODE).to(device)
    if not encoder.HipGeometryEncoder.supports(cfg.img_resolution):
        raise RuntimeError(f"the geometry-encoder kernels tile patches of 32, 64 or 128 k pixels; this checkpoint paints {cfg.img_resolution}")
    ops = painting.TileOps(G, encoder.HipGeometryEncoder(enc_sd, preproc_type=preproc, device=device))
    from .drawings import load_calibration
    mapper = painting.StyleUVSMapper(ops, *load_calibration(args.uvs_calibration, cfg.img_resolution, device))
    library = formats.BrushLibrary.from_arg(args.library, z_dim=G.z_dim)
    with torch.no_grad():
        cat = mapper.catalogue(library, batch=args.batch, icon_k=args.icon_k)
    sheet, info = write_catalogue(cat, args.output_file_prefix, args.cols)
    logger.info(f"Saved {len(cat.ids)} brushes to: {sheet}, {info}")
    print(sheet)
    print(info)
    return sheet, info


if __name__ == "__main__":
    main()
