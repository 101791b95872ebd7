"""Golden vectors for the brush catalogue: the REFERENCE StyleUVSMapper (forger/ui/mapper.py:74-136) on the R=128 engine of
make_golden_engine.py -- get_colors_raw, get_colors, get_brush_icon (on white and plain) and get_sfactor of four brushes: z seeds
594, 0 and 1, and one W+ brush (mapping(z_7) handed to set_style_w).  The calibration drawings are the synthetic ones already stored
in engine_r128.npz.  Build container only.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_brush_catalogue.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
import make_golden_engine as mge  # noqa: E402  (puts the reference and its stubs on the path, then imports it)

brush = mge.brush

Z_SEEDS = (594, 0, 1)
W_SEED = 7


def install_calibration(eng, medium, thick):
    """What StyleUVSMapper._init_geometry (mapper.py:24-44) does with the bundled drawings, on the stored stand-ins."""
    mapper = eng.uvs_mapper
    geo_input = (torch.from_numpy(medium).to(torch.float32) / 255).unsqueeze(1)
    mapper.geom_feature = eng.encoder.encode(geo_input)
    mapper.fmask = geo_input < 0.01
    mapper.bmask = (torch.from_numpy(thick).to(torch.float32) / 255).unsqueeze(1) > 0.99
    return mapper


def main():
    R = 128
    eng = mge.build_engine(R)
    with np.load(os.path.join(HERE, "engine_r128.npz")) as g:
        medium, thick, sf594 = g["uvs_cal_medium"], g["uvs_cal_thick"], np.float32(g["uvs_sfactor"])
    mapper = install_calibration(eng, medium, thick)
    brushes = []
    for seed in Z_SEEDS:
        opts = brush.GanBrushOptions()
        opts.set_style(eng.random_style(seed), seed)
        brushes.append(opts)
    with torch.no_grad():
        w = eng.G.mapping(eng.random_style(W_SEED).to(torch.float32), None)
    opts = brush.GanBrushOptions()
    opts.set_style_w(w, "w%d" % W_SEED)
    brushes.append(opts)
    out = {"resolution": np.int64(R), "weights_seed": np.int64(0), "encoder_seed": np.int64(5), "z_seeds": np.array(Z_SEEDS, np.int64),
           "w_seed": np.int64(W_SEED), "w_brush_ws": w.numpy()}
    colors, specs, white, plain, sfs = [], [], [], [], []
    with torch.no_grad():
        for opts in brushes:
            colors.append(mapper.get_colors_raw(opts).numpy()[0])
            specs.append(mapper.get_colors(opts))
            white.append(mapper.get_brush_icon(opts, on_white=True))
            plain.append(mapper.get_brush_icon(opts, on_white=False))
            sfs.append(np.float32(mapper.get_sfactor(opts)))
    assert sfs[0] == sf594, (sfs[0], sf594)                 # the factor engine_r128.npz holds for brush 594
    out["colors_raw"] = np.stack(colors).astype(np.float32)
    out["color_specs"] = np.array(specs)
    out["icons_on_white"], out["icons_plain"] = np.stack(white), np.stack(plain)
    out["sfactors"] = np.array(sfs, np.float32)
    path = os.path.join(HERE, "brush_catalogue_r128.npz")
    np.savez_compressed(path, **out)
    print("brush_catalogue_r128.npz:", {k: getattr(v, "shape", None) for k, v in out.items()}, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
