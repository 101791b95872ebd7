"""The stitching scores' inputs, stated in numpy: what ``nb_stitch_crops_u8`` and ``nb_stitch_pairs_f32`` (csrc/nb_stitch_metrics.hip)
and their torch restatements in ``TileOpsBase`` must give, written from the reference lines they replace
(forger/train/stitching.py:161-179, 248-253; forger/metrics/geom_metric.py:165-187; metric_main.py:181-189), the cases shared by the
CPU and GPU tests, and the tolerances.

Tolerances.  The pair buffer and the crops hold COPIES (of an input float; of value / 255 correctly rounded to float32), so both are
held to exact equality with the float32 statement.  An L1 sum is held to ``(c + 1) * 2^-24 * sum |terms|`` of the float64 sum of the
float32 inputs' differences: every term |a - b| is one rounded subtraction (relative error 2^-24, the "+ 1"), and ``c`` is the longest
chain of additions a sum goes through in the kernel, ``chain(s)`` below."""
import numpy as np
import torch

EPS32 = 2.0 ** -24
PARTS = 32                                 # NB_STITCH_PARTS
THREADS = 256


def chain(s: int) -> int:
    """The longest chain of float32 additions behind one sum of ``nb_stitch_pairs_f32`` at crop width ``s``.  A sample's work items
    (G consecutive columns of one row of one plane: 3 * s * ceil(s / G) of them, G = 4 on the 16-byte path and 1 otherwise) are dealt
    to PARTS workgroups of THREADS threads; a thread adds its items' terms one after the other -- G * ceil(ceil(items / PARTS) /
    THREADS) additions --; then 6 halving steps across the 64 lanes of a wave, 3 additions for the other three waves, and PARTS - 1
    additions in the finish.  The larger of the two paths is taken, so one bound holds for every layout.  (The torch restatement's
    pairwise sums have shorter chains.)"""
    cd = lambda a, b: -(-a // b)
    per_thread = max(4 * cd(cd(3 * s * cd(s, 4), PARTS), THREADS), cd(cd(3 * s * s, PARTS), THREADS))
    return per_thread + 6 + 3 + (PARTS - 1)


# ---------------------------------------------------------------------------------------------------------------------
# the crops
# ---------------------------------------------------------------------------------------------------------------------
def u8_over_255() -> np.ndarray:
    """[256] float32: v / 255 correctly rounded, from the exact quotient (float64 division, itself within 2^-53, is far from every
    float32 rounding boundary for these 256 values: asserted by the CPU test against the rational)."""
    return (np.arange(256, dtype=np.float64) / 255.0).astype(np.float32)


def crop_cases():
    """D = 40 and D = 33 at R = 32 (16-byte rows), R = 30 in D = 33 (rows that are not): windows at both extremes of their range and
    between, drawing indices out of order and repeated."""
    out = []
    for name, k, d, r, seed in (("d40_r32", 3, 40, 32, 1), ("d33_r32", 2, 33, 32, 2), ("d33_r30", 4, 33, 30, 3)):
        rs = np.random.RandomState(seed)
        drawings = rs.randint(0, 256, (k, d, d)).astype(np.uint8)
        drawings[0, :2] = np.arange(2 * d).reshape(2, d) % 256             # every byte value occurs
        lim = d - r
        off = np.array([[0, 0], [lim, lim], [0, lim], [lim, 0], [lim // 2, lim - 1], [1, lim // 2]], np.int32)
        draw = np.array([k - 1, 0, k - 1, 1 % k, 0, k // 2], np.int32)
        out.append(dict(name=name, drawings=drawings, draw=draw, off=off, r=r))
    return out


def crop_statement(c) -> np.ndarray:
    """[n,1,r,r] float32 (metric_main.py:183-189: ``geom.to(float32) / 255.0`` cropped at (row, column))."""
    lut, r = u8_over_255(), c["r"]
    return np.stack([lut[c["drawings"][j, y:y + r, x:x + r]] for j, (y, x) in zip(c["draw"].tolist(), c["off"].tolist())])[:, None]


# ---------------------------------------------------------------------------------------------------------------------
# the pairs
# ---------------------------------------------------------------------------------------------------------------------
def rect_kinds(r: int, m: int):
    """{kind: (area in the destination, area in the source)} as (rstart, cstart, rend, cend), ends exclusive, for r x r images whose crop
    window is rows and columns m .. r - 2 m.  Needs r >= 30."""
    w0, w1 = m, r - 2 * m
    mk = lambda r0, c0, h, w, sr0, sc0: ((r0, c0, r0 + h, c0 + w), (sr0, sc0, sr0 + h, sc0 + w))
    kinds = {
        "inside": mk(w0 + 3, w0 + 5, 7, 9, w0 + 5, w0 + 1),
        "top": mk(0, 4, w0 + 4, 11, r - w0 - 4, 1),
        "bottom": mk(w1 - 3, 6, r - w1 + 3, 14, 0, 9),
        "left": mk(5, 0, 12, w0 + 6, 7, r - w0 - 6),
        "right": mk(8, w1 - 2, 13, r - w1 + 2, 3, 0),
        "one_wide": mk(w0 + 1, w0 + 7, 15, 1, 2, 0),
        "one_high": mk(w0 + 9, w0 + 2, 1, 13, r - 1, 4),
        "whole": mk(0, 0, r, r, 0, 0),
        "empty": ((0, 0, 0, 0), (0, 0, 0, 0)),
        "negative": ((10, 10, 5, 20), (12, 3, 7, 13)),                     # negative extent: nothing is composited
        "leaves": ((0, 0, r + 1, r), (0, 0, r + 1, r)),                    # leaves the image: the kernel composites nothing
        "mismatch": ((2, 2, 10, 10), (2, 2, 10, 11)),                      # extents differ: likewise
    }
    if m > 0:                                                              # wholly outside the window: in the strips the crop removes
        kinds["outside_top"] = mk(0, 0, m, r, r - m, 0)
        kinds["outside_bottom"] = mk(w1, 3, r - w1, 9, 4, 11)
        kinds["outside_right"] = mk(3, w1, 9, r - w1, 11, 2)
    return kinds


def _case(name, r, m, kinds_a, kinds_b, seed):
    kinds = rect_kinds(r, m)
    n = len(kinds_a)
    rs = np.random.RandomState(seed)
    fake = rs.randn(2 * n, 3, r, r).astype(np.float32)
    # (area1, area2) per sample.  First composite: area1 in fake1 takes fake2's area2.  Second: area2 in fake2 takes fake1's area1.
    rects_a = np.array([kinds[q][0] + kinds[q][1] for q in kinds_a], np.int32)
    rects_b = np.array([kinds[q][1] + kinds[q][0] for q in kinds_b], np.int32)
    return dict(name=name, r=r, margin=m, n=n, fake=fake, rects_a=rects_a, rects_b=rects_b)


def pair_cases():
    """R = 32 with margin 2 (S = 26, not a multiple of four): every kind of rectangle alone at n = 1, and n = 5 with rectangles that
    differ from sample to sample; margin 0 (S = R: nothing lies outside), margin 4 (S = 20: the 16-byte path with an inset window) and
    margin 1 (S = 29, odd) at R = 32; R = 33 with margin 1 (S = 30, rows that start at odd addresses); R = 256 with margin 10, n = 1
    (S = 226, the painting size) with the rectangles of a real crop pair."""
    out = []
    names = sorted(rect_kinds(32, 2))
    for i, q in enumerate(names):
        out.append(_case(f"r32_m2_n1_{q}", 32, 2, [q], [names[(i + 5) % len(names)]], 10 + i))
    out.append(_case("r32_m2_n5", 32, 2, ["inside", "top", "empty", "right", "outside_top"], ["bottom", "whole", "left", "one_wide", "inside"], 40))
    out.append(_case("r32_m0_n5", 32, 0, ["inside", "top", "whole", "right", "negative"], ["bottom", "one_high", "left", "empty", "inside"], 41))
    out.append(_case("r32_m0_n1", 32, 0, ["left"], ["one_wide"], 42))
    out.append(_case("r32_m4_n5", 32, 4, ["inside", "outside_bottom", "left", "bottom", "leaves"], ["top", "right", "outside_right", "mismatch", "one_wide"], 43))
    out.append(_case("r32_m1_n5", 32, 1, ["right", "inside", "outside_top", "one_high", "bottom"], ["whole", "left", "top", "inside", "empty"], 44))
    out.append(_case("r33_m1_n5", 33, 1, ["inside", "top", "bottom", "left", "right"], ["one_wide", "outside_bottom", "whole", "inside", "negative"], 45))
    out.append(_case("r33_m1_n1", 33, 1, ["whole"], ["right"], 46))
    big = _case("r256_m10_n1", 256, 10, ["inside"], ["inside"], 47)
    big["rects_a"], big["rects_b"] = (q[None] for q in crop_pair_rects((40, 100, 256, 256), (117, 21, 256, 256), 10))
    out.append(big)
    return out


def crop_pair_rects(crop1, crop2, margin):
    """(rects_a [8], rects_b [8]) int32 of two crops (row, column, height, width): ``compute_overlaps(crop1, offset_crop(crop2))`` and
    ``compute_overlaps(offset_crop(crop1), crop2)`` (stitching.py:50-83, 248, 252) written out; zeros without an overlap."""
    def overlaps(a, b):
        r0, c0, r1, c1 = max(a[0], b[0]), max(a[1], b[1]), min(a[0] + a[2], b[0] + b[2]), min(a[1] + a[3], b[1] + b[3])
        if min(r1 - r0, c1 - c0) <= 0:
            return [0] * 8
        return [r0 - a[0], c0 - a[1], r1 - a[0], c1 - a[1], r0 - b[0], c0 - b[1], r1 - b[0], c1 - b[1]]
    inset = lambda c: (c[0] + margin, c[1] + margin, c[2] - 2 * margin, c[3] - 2 * margin)
    return np.array(overlaps(crop1, inset(crop2)), np.int32), np.array(overlaps(inset(crop1), crop2), np.int32)


def _valid(dst, src, r):
    r0, c0, r1, c1 = dst
    return (0 <= r0 < r1 <= r and 0 <= c0 < c1 <= r and src[0] >= 0 and src[2] <= r and src[1] >= 0 and src[3] <= r
            and src[2] - src[0] == r1 - r0 and src[3] - src[1] == c1 - c0)


def pair_statement(fake: np.ndarray, rects_a: np.ndarray, rects_b: np.ndarray, margin: int):
    """(x [4n,3,S,S] float32, l1 [2n] float64) of ``fake`` [2n,3,R,R] float32.  fake1_composite = fake1 with the pixels of area2 of
    fake2 in area1 (``composite``: mask1 zero on area1, ``mask1 * im1``, then ``+=`` the other's patch -- for finite values a copy);
    fake2_composite = fake2 with fake1's area1 in area2 (stitching.py:248-253); all four cropped ``[margin:R - 2 margin]`` on both
    axes (geom_metric.py:173-177; margin 0: uncropped); l1 = sum |first - second| over a pair's 3 S S entries."""
    n, r, m = fake.shape[0] // 2, fake.shape[-1], int(margin)
    f1, f2 = fake[:n], fake[n:]
    c1, c2 = f1.copy(), f2.copy()
    for i in range(n):
        a1, a2 = rects_a[i, :4].tolist(), rects_a[i, 4:].tolist()
        if _valid(a1, a2, r):
            c1[i, :, a1[0]:a1[2], a1[1]:a1[3]] = f2[i, :, a2[0]:a2[2], a2[1]:a2[3]]
        b1, b2 = rects_b[i, :4].tolist(), rects_b[i, 4:].tolist()
        if _valid(b2, b1, r):
            c2[i, :, b2[0]:b2[2], b2[1]:b2[3]] = f1[i, :, b1[0]:b1[2], b1[1]:b1[3]]
    crop = (lambda t: t) if m == 0 else (lambda t: t[:, :, m:r - 2 * m, m:r - 2 * m])
    x = np.ascontiguousarray(np.concatenate([crop(f1), crop(f2), crop(c1), crop(c2)]))
    l1 = np.abs(x[:2 * n].astype(np.float64) - x[2 * n:].astype(np.float64)).sum(axis=(1, 2, 3))
    return x, l1


def statement(c):
    return pair_statement(c["fake"], c["rects_a"], c["rects_b"], c["margin"])


def l1_bound(l1_f64: np.ndarray, s: int) -> np.ndarray:
    """(c + 1) * 2^-24 * sum |terms| with c = ``chain(s)``: the terms are not negative, so their absolute sum is the sum itself."""
    return (chain(s) + 1) * EPS32 * np.abs(l1_f64)


def check_pairs(x: np.ndarray, l1: np.ndarray, c, what=None) -> float:
    """The buffer equal to the statement as bytes, every sum within ``l1_bound``; returns the largest error / bound."""
    want_x, want_l1 = statement(c)
    assert x.shape == want_x.shape and x.dtype == np.float32 and x.tobytes() == want_x.tobytes(), (c["name"], what)
    s = want_x.shape[-1]
    err, tol = np.abs(l1.astype(np.float64) - want_l1), l1_bound(want_l1, s)
    assert l1.shape == want_l1.shape and np.all(err <= tol), (c["name"], what, l1, want_l1, tol)
    return float((err / np.maximum(tol, 1e-300)).max())


def to_torch(c, device="cpu"):
    return tuple(torch.from_numpy(c[k]).to(device) for k in ("fake", "rects_a", "rects_b"))


# (arch, S): R, margin, and the seed of the images.  The images are tanh(randn), the spread lpips_refs.SLIM's weights were normalised
# on; one sample, so two pairs.  No seed keeps every ReLU and pool decision lpips_refs.KINK_MARGIN float32-route errors from zero at
# these sizes (of seeds 0..11 only alex at S = 52 holds it: 226 x 226 images have too many activations for the smallest of them to
# stay that far out), so the margins are not a condition here; ReLU and max are continuous, so a decision that falls the other way
# moves the distance by no more than the error that flipped it, which the tolerance's factor covers.
DISTANCE_CASES = {("alex", 52): dict(r=64, margin=4, seed=0), ("alex", 226): dict(r=256, margin=10, seed=0),
                  ("vgg", 52): dict(r=64, margin=4, seed=0), ("vgg", 226): dict(r=256, margin=10, seed=0)}


def distance_case(arch: str, s: int, seed=None):
    """A pair case of one sample for ``pair_distance`` at crop width ``s``, with the rectangles of a real crop pair."""
    d = DISTANCE_CASES[(arch, s)]
    r, m = d["r"], d["margin"]
    rs = np.random.RandomState(900 + (d["seed"] if seed is None else seed))
    fake = np.tanh(rs.randn(2, 3, r, r)).astype(np.float32)
    ra, rb = crop_pair_rects((r // 8, r // 3, r, r), (r // 8 + r // 4, r // 3 - r // 5, r, r), m)
    assert r - 3 * m == s
    return dict(name=f"distance_{arch}_{s}", r=r, margin=m, n=1, fake=fake, rects_a=ra[None], rects_b=rb[None])


def scores_from_fake(fake: np.ndarray, rects_a, rects_b, margin: int, ks: int, dist):
    """(STITCH_L1 [nu], STITCH_LPIPS [nu]) float64 of one pass's ``fake`` [2 nu ks,3,R,R]: per unit 0.5 * (first + second direction),
    LPIPS the mean over the unit's ks samples of ``dist(x) -> [2n]``, L1 the mean over ks * 3 * S * S entries
    (geom_metric.py:179-187)."""
    x, l1 = pair_statement(fake, np.asarray(rects_a), np.asarray(rects_b), margin)
    n, s = fake.shape[0] // 2, x.shape[-1]
    d = np.asarray(dist(x), np.float64)
    per = lambda v: v.reshape(n // ks, ks)
    return (0.5 * (per(l1[:n]).sum(axis=1) + per(l1[n:]).sum(axis=1)) / (ks * 3 * s * s),
            0.5 * (per(d[:n]).mean(axis=1) + per(d[n:]).mean(axis=1)))
