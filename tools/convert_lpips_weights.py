#!/usr/bin/env python
"""Write the ``.npz`` that ``brushstroke_engine_amd.perceptual.LPIPS`` loads, from the two weight files a user has:

    python tools/convert_lpips_weights.py --trunk vgg16-397923af.pth --head vgg.pth --arch vgg --out lpips_vgg.npz

``--trunk``: the ``torch.save``d state dict of torchvision's ``vgg16`` or ``alexnet`` (``features.N.weight`` / ``features.N.bias``).
``--head``: the LPIPS package's linear heads for that trunk (``lin<l>.model.1.weight``, ``[1,C,1,1]``).  Neither torchvision nor the
``lpips`` package is needed.  The result holds ``features.<i>.weight`` / ``.bias`` of the convolutions, ``lin<l>.weight`` ``[C_l]``,
``arch`` and the scaling layer's constants.  No weights ship with the project."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from brushstroke_engine_amd.perceptual import convert_state_dicts  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--trunk", required=True, help="torchvision state dict (.pth)")
    ap.add_argument("--head", required=True, help="LPIPS linear heads (.pth)")
    ap.add_argument("--arch", required=True, choices=("vgg", "alex"))
    ap.add_argument("--out", required=True, help=".npz to write")
    args = ap.parse_args(argv)
    load = lambda p: torch.load(p, map_location="cpu", weights_only=True)
    entries = convert_state_dicts(load(args.trunk), load(args.head), args.arch)
    np.savez(args.out, **entries)
    print(args.out)
    return args.out


if __name__ == "__main__":
    main()
