"""Golden vectors for the stitching scores: the REFERENCE's ``RandomStitcher.generate_with_stitching`` (forger/train/stitching.py) and
``compute_stitching_metrics`` (forger/metrics/geom_metric.py:165-187) on seeded images at R = 32, N = 2, margins 0 and 3.  The LPIPS
network is replaced by a recorder: the fixture holds the tensors the reference hands to it -- which pins the asymmetric crop and the
composites -- and the STITCH_L1 it returns, which pins the normalisation.  Build container only.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_stitch_metrics.py
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, "/root/reference")
tv = types.ModuleType("torchvision"); tvt = types.ModuleType("torchvision.transforms"); tv.transforms = tvt
sys.modules.update({"torchvision": tv, "torchvision.transforms": tvt})
for name in ("skimage", "skimage.io", "skimage.filters", "skimage.morphology", "lpips"):
    sys.modules.setdefault(name, types.ModuleType(name))
import thirdparty.stylegan2_ada_pytorch  # noqa: E402,F401
import forger.metrics.geom_metric as GM  # noqa: E402
import forger.train.stitching as S  # noqa: E402

R, N = 32, 2
CROP1, CROP2 = (10, 12, R, R), (17, 5, R, R)
MIN_OVERLAP = 6


def main():
    rs = np.random.RandomState(23)
    # multiples of 1/4 in -2..2: exact in float32, and the archive stays small
    fakes = [torch.from_numpy((rs.randint(-8, 9, (N, 3, R, R)) / 4.0).astype(np.float32)) for _ in range(2)]
    out = {"fake1": fakes[0].numpy(), "fake2": fakes[1].numpy(), "crop1": np.array(CROP1), "crop2": np.array(CROP2),
           "min_overlap": np.int64(MIN_OVERLAP), "margins": np.array([0, 3])}

    class FakeG:
        img_resolution = R

        def __init__(self):
            self.calls = []

        def __call__(self, z, c, geom_feature, positions=None, style_mixing_prob=0):
            self.calls.append(positions.clone())
            return fakes[len(self.calls) - 1].clone()

    for margin in (0, 3):
        seen = []

        def recorder(im1, im2):
            seen.append((im1.clone(), im2.clone()))
            return (im1 - im2).abs().mean(dim=(1, 2, 3)) * 2 + 1           # a fixed simple function of what it is handed

        GM.lpips_batched = recorder
        g = FakeG()
        st = S.RandomStitcher(crop_margin=margin, min_overlap=MIN_OVERLAP)
        pos1 = torch.from_numpy(rs.randint(0, R - 1, (N, 2)).astype(np.int64))
        res = st.generate_with_stitching(g, torch.zeros(N, 4), None, None, None, CROP1, CROP2, positions1=pos1)
        got = GM.compute_stitching_metrics(res, margin=margin)
        assert len(seen) == 2 and torch.equal(g.calls[1] - g.calls[0], torch.tensor([[CROP2[0] - CROP1[0], CROP2[1] - CROP1[1]]]).expand(N, 2))
        p = f"m{margin}_"
        out.update({p + "positions1": pos1.numpy(), p + "positions2": res["positions2"].numpy(),
                    p + "lpips_a0": seen[0][0].numpy(), p + "lpips_a1": seen[0][1].numpy(),
                    p + "lpips_b0": seen[1][0].numpy(), p + "lpips_b1": seen[1][1].numpy(),
                    p + "STITCH_L1": np.float64(float(got["STITCH_L1"])), p + "STITCH_LPIPS": np.float64(float(got["STITCH_LPIPS"]))})
        print(margin, tuple(seen[0][0].shape), float(got["STITCH_L1"]), float(got["STITCH_LPIPS"]))
    path = os.path.join(HERE, "stitch_metrics.npz")
    np.savez_compressed(path, **out)
    print("stitch_metrics.npz:", len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
