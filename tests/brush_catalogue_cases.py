"""Inputs and the numpy statement for ``masked_kth_largest`` (TEST ONLY): shared by the torch route's test on the CPU and the
kernel's test on the GPU, so both are held to the same cases."""
import numpy as np

COUNTS = (1, 255, 256, 257, 1089, 16384)


def kth_largest_numpy(x, masks, k):
    """(kth [n] float32, n_masked [n] int32) of x [n,count] float32 and masks [m,count]: a stable sort of the included values, NaN on
    top (``np.sort`` puts every NaN last, and -0 == +0), no float64 anywhere."""
    n, m = x.shape[0], masks.shape[0]
    kth, cnt = np.full([n], np.nan, np.float32), np.zeros([n], np.int32)
    for i in range(n):
        v = np.sort(x[i][masks[i % m] != 0], kind="stable")
        cnt[i] = v.size
        if v.size >= k:
            kth[i] = v[v.size - k]
    return kth, cnt


def _ks(masks, n, extra=()):
    """k = 1, 15, the smallest n_masked of the images, and one more than that (NaN there, the count still reported)."""
    nm = min(int((masks[i % masks.shape[0]] != 0).sum()) for i in range(n))
    return sorted({k for k in (1, 15, nm, nm + 1) + tuple(extra) if k >= 1})


def special_mix(count=257):
    """-inf, +inf, +-0, denormals, negatives and NaNs (both signs, with payloads) among finite values."""
    rs = np.random.RandomState(5)
    v = (rs.randn(count) * 3).astype(np.float32)
    bits = v.view(np.uint32)
    bits[0:3] = (0x7fc00000, 0xffc00001, 0x7f800123)          # three NaNs
    v[3:5] = np.inf
    v[5:7] = -np.inf
    v[7:10] = 0.0
    bits[10:13] = 0x80000000                                  # -0
    bits[13:15] = (0x00000001, 0x007fffff)                    # denormals
    bits[15:17] = (0x80000001, 0x807fffff)
    return v[rs.permutation(count)].copy()


def cases():
    """[(name, x [n,count] float32, masks [m,count] uint8, [k, ...])]"""
    rs = np.random.RandomState(0)
    out = []
    for j, count in enumerate(COUNTS):                        # random normals at every size, one and five masks
        m = 1 if j % 2 else 5
        masks = (rs.rand(m, count) < 0.5).astype(np.uint8) if count > 1 else np.ones([m, 1], np.uint8)
        out.append((f"normal_c{count}_m{m}", rs.randn(5, count).astype(np.float32), masks, _ks(masks, 5)))
    masks = (rs.rand(5, 257) < 0.3).astype(np.uint8)          # more workgroups than CUs, i % n_masks wrapping
    out.append(("normal_n300", rs.randn(300, 257).astype(np.float32), masks, _ks(masks, 300)))
    masks = (rs.rand(5, 1089) < 0.5).astype(np.uint8)
    out.append(("normal_n7", rs.randn(7, 1089).astype(np.float32), masks, _ks(masks, 7)))
    masks = (rs.rand(1, 16384) < 0.9).astype(np.uint8)
    out.append(("normal_n1", rs.randn(1, 16384).astype(np.float32), masks, _ks(masks, 1)))
    count = 1089
    ones = np.ones([1, count], np.uint8)
    out.append(("all_equal", np.full([5, count], 0.73, np.float32), ones, _ks(ones, 5)))
    two = np.full([5, count], 0.25, np.float32)               # two values; image i holds 13 + i of the larger: k = 15 on both sides
    for i in range(5):
        two[i, rs.permutation(count)[:13 + i]] = 0.75
    out.append(("two_values", two, ones, [13, 14, 15, 16, 17, 18]))
    logits = rs.randn(5, 3, count).astype(np.float32) * 4
    e = np.exp(logits - logits.max(axis=1, keepdims=True))
    soft = (e / e.sum(axis=1, keepdims=True))[:, 2].astype(np.float32)
    soft = ((soft.view(np.uint32) & np.uint32(0xffff)) | np.uint32(0x3f7a0000)).view(np.float32)       # (0,1), the high 16 bits shared
    masks = (rs.rand(5, count) < 0.5).astype(np.uint8)
    out.append(("softmax_shared_high_bits", soft, masks, _ks(masks, 5)))
    mix = np.stack([special_mix(257) for _ in range(2)])
    mix[1] = mix[1][::-1]
    ones257 = np.ones([1, 257], np.uint8)
    desc = np.sort(mix[0])[::-1]                              # NaN, NaN, NaN, inf, inf, finite ... 0 ... -inf
    k_zero = int(np.flatnonzero(desc == 0)[2]) + 1
    out.append(("special_mix", mix, ones257, [1, 3, 4, 5, 6, k_zero, 255, 257, 258]))
    for count in (257, 1089):                                 # mask shapes
        x = rs.randn(5, count).astype(np.float32)
        out.append((f"mask_ones_c{count}", x, np.ones([1, count], np.uint8), [1, 15, count, count + 1]))
        out.append((f"mask_zeros_c{count}", x, np.zeros([1, count], np.uint8), [1, 15]))
        exact = np.zeros([5, count], np.uint8)
        for i in range(5):
            exact[i, rs.permutation(count)[:15]] = 1 + i      # any non-zero byte includes
        out.append((f"mask_exactly_k_c{count}", x, exact, [15, 16]))
        last = np.zeros([1, count], np.uint8)
        last[0, count - 3:] = 1                               # only the elements behind the last whole vector of an aligned row
        out.append((f"mask_last_partial_c{count}", x, last, [1, 3, 4]))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the four brushes of tests/golden/brush_catalogue_r128.npz
# ---------------------------------------------------------------------------------------------------------------------
class FixtureLibrary:
    """The fixture's brushes as a library: z seeds 594, 0 and 1, and the W+ brush."""

    def __init__(self, g, z_dim):
        self.g, self.z_dim = g, z_dim

    def get_style_ids(self):
        return [str(s) for s in self.g["z_seeds"].tolist()] + ["w%d" % int(self.g["w_seed"])]

    def set_style(self, style_id, brush_options):
        import torch
        if str(style_id).startswith("w"):
            brush_options.set_style_w(torch.from_numpy(self.g["w_brush_ws"]), style_id)
        else:
            brush_options.set_style(torch.from_numpy(np.random.RandomState(int(style_id)).randn(1, self.z_dim)), style_id)


def canvas_close(a, b, max_frac=1e-3):
    """The project's canvas condition (``_canvas_close`` of tests/test_hip_painting.py): every byte within 1, at most ``max_frac`` differ."""
    d = np.abs(a.astype(np.int32) - b.astype(np.int32))
    assert a.shape == b.shape and d.max() <= 1, d.max()
    assert (d > 0).mean() <= max_frac, (d > 0).sum()


def spec_ints(spec):
    import re
    return np.array([int(x) for x in re.findall(r"\d+", spec)])
