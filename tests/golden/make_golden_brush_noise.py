"""Golden vectors for a PROJECTED brush (a W+ code plus a noise_const replacement for every synthesis layer, what the reference's
brush libraries store: forger/ui/library.py:146-202): the REFERENCE PaintingHelper.render_stroke (forger/ui/brush.py:244-398) on CPU
for two overlapping R=128 tiles at feature-blending level 2, crop margin 10, with the brush set through
``set_style_w(ws, custom_args={'noise_buffers': ...})`` -- and the same two tiles without the buffers.  Build container only.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_brush_noise.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_engine import brush, build_engine, stroke_sequence  # noqa: E402

from brushstroke_engine_amd import config as cfgmod  # noqa: E402

R, CROP, SIZE, LEVEL = 128, 10, 256, 2
NOISE_SEED, NOISE_SCALE, STYLE_SEED = 2024, 1.0, 594
XY = [(24, 16), (88, 72)]                 # (x, y) of the two tiles: they overlap in a 64 x 72 region


def noise_buffers(cfg, seed=NOISE_SEED, scale=NOISE_SCALE):
    """Seeded normals for every layer under the reference's key names (tests/test_brush_noise_cpu.py restates this)."""
    rs = np.random.RandomState(seed)
    return {f"b{s.block_res}.conv{0 if s.up == 2 else 1}.noise_const": (rs.randn(s.block_res, s.block_res) * scale).astype(np.float32)
            for s in cfg.layers}


def paint(eng, ws, patches, custom_args):
    helper = brush.PaintingHelper(eng, style_seed=0)
    helper.make_new_canvas(SIZE, SIZE, feature_blending=LEVEL)
    helper.set_render_mode("clear")
    triads, inner = [], eng._render_stroke_torch

    def spy(*a, **k):
        out = inner(*a, **k)
        triads.append(out[1])
        return out
    eng._render_stroke_torch = spy
    tiles = []
    try:
        with torch.no_grad():
            for (x, y), patch in zip(XY, patches):
                opts = brush.GanBrushOptions()
                opts.set_style_w(ws.clone(), STYLE_SEED, custom_args=custom_args)
                opts.set_position(x, y)
                res, _, meta = helper.render_stroke(patch, None, opts, meta={"x": x, "y": y, "crop_margin": CROP})
                tiles.append(res)
    finally:
        eng._render_stroke_torch = inner
    return np.stack(tiles), triads


def main():
    cfg = cfgmod.style1_config(R)
    eng = build_engine(R)
    patches = [p for _, _, p, _ in stroke_sequence(R, n_strokes=2, seed=23, size=SIZE)]
    with torch.no_grad():
        ws = eng.G.mapping(eng.random_style(STYLE_SEED), None)
    bufs = noise_buffers(cfg)
    with_noise, triads = paint(eng, ws, patches, {"noise_buffers": {k: torch.from_numpy(v.copy()) for k, v in bufs.items()}})
    without, _ = paint(eng, ws, patches, None)
    d = np.abs(with_noise.astype(np.int32) - without.astype(np.int32))
    print(f"with vs without buffers: {(d > 1).mean():.3f} of the bytes differ by more than 1 LSB (max {d.max()})")
    assert (d > 1).mean() > 0.05
    out = {"resolution": np.int64(R), "crop_margin": np.int64(CROP), "size": np.int64(SIZE), "level": np.int64(LEVEL),
           "weights_seed": np.int64(0), "encoder_seed": np.int64(5), "noise_seed": np.int64(NOISE_SEED), "noise_scale": np.float64(NOISE_SCALE),
           "xy": np.array(XY, np.int64), "patches": np.packbits(np.stack([p[..., 0] for p in patches]) > 0),
           "ws": ws.numpy().astype(np.float32), "tiles_noise": with_noise, "tiles_plain": without,
           "uvs0": triads[0]["uvs"].numpy().astype(np.float32), "colors0": triads[0]["colors"].numpy().astype(np.float32)}
    path = os.path.join(HERE, "engine_brush_noise_r128.npz")
    np.savez_compressed(path, **out)
    print("engine_brush_noise_r128.npz:", {k: getattr(v, "shape", None) for k, v in out.items()}, os.path.getsize(path), "bytes;",
          "engine_r128.npz:", os.path.getsize(os.path.join(HERE, "engine_r128.npz")), "bytes")
    assert os.path.getsize(path) < os.path.getsize(os.path.join(HERE, "engine_r128.npz"))


if __name__ == "__main__":
    main()
