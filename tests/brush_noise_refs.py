"""What the brush-noise tests share: the inputs of tests/golden/engine_brush_noise_r128.npz rebuilt from what the fixture stores."""
import numpy as np


def fixture_buffers(g, cfg):
    """tests/golden/make_golden_brush_noise.py's noise_buffers, from the stored seed and scale."""
    rs = np.random.RandomState(int(g["noise_seed"]))
    return {f"b{s.block_res}.conv{0 if s.up == 2 else 1}.noise_const":
            (rs.randn(s.block_res, s.block_res) * float(g["noise_scale"])).astype(np.float32) for s in cfg.layers}


def fixture_patches(g):
    R = int(g["resolution"])
    return (np.unpackbits(g["patches"])[:2 * R * R].reshape(2, R, R, 1) * 255).astype(np.uint8)
