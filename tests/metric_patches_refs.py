"""A float64 numpy statement of the inputs of the perceptual brush scores (csrc/nb_metric_patches.hip, ``TileOpsBase.bg_guidance`` /
``bg_mean_colors`` / ``metric_pairs``) and of the scores themselves, with the cases their tests share (TEST ONLY).

Neither ``lpips`` nor ``torchvision`` is in the tree, so the reference's ``compute_uniform_bg_lpips_metric``
(forger/metrics/geom_metric.py:207-262) and ``compute_lpips_across_geo`` (geom_metric.py:190-204) cannot make fixtures; like
tests/lpips_refs.py this statement is written from the cited lines.  It builds on tests/brush_metrics_refs.py (the blur, the drawings
and renders of ``cases()``, whose inputs are exact in float32) and tests/lpips_refs.py (the network in float64, slim weights, bounds)."""
import numpy as np
import torch

import brush_metrics_refs as br
import lpips_refs as lr

BG_THRESH = 0.99                       # geom_metric.py:238, on the guidance blurred ONCE (line 235)
UNDECIDED = 1e-5                       # a pixel whose float64 blur lies this close to BG_THRESH may fall on either side in fp32
UNDECIDED_CAP = 1e-3                   # ... and at most this share of a drawing's pixels may be undecided
U = 2.0 ** -24                         # unit roundoff of float32
# One fp32 pass of <= 25 products and sums of values in 0..1, counted as BLUR_TOL of brush_metrics_refs counts its two passes
# (2 * 26 * 2^-24 = 3.1e-6, stated as 4e-6): one pass is 26 * 2^-24 = 1.55e-6, stated as
BLUR1_TOL = 2e-6
# A pixel of the output that keeps its colour: a * c (U), 1 - a (U), their sum (U, value <= 1), then * 2 (exact) doubles the 3 U, and
# - 1 rounds once more (value in -1..1): 7 U.  "A few ulps of 1": 8 U = 4 ulps of a value in 0.5..1.
PIXEL_TOL = 8 * U
# The mean colour: per pixel the composite's 3 U; the sum of N values in 0..1 in ANY order whose longest chain of additions is d deep
# errs by at most d U relative to the sum (all terms are non-negative, so nothing cancels).  The kernel's order is fixed: a thread adds
# ceil(N / (16 * 256 * v)) groups of v values (v = 4 or 1; 1 group at the sizes of the cases, 4 values at most), 6 shuffle levels, 3
# waves, 15 partials: d <= 28 here; torch's sum is pairwise in blocks, shallower.  d = 64 covers both and any r up to 256 (16 + 6 + 3 +
# 15 = 40).  The quotient adds U, the count is an exact integer.  Relative to the value, which lies in 0..1:
MEAN_TOL = (3 + 64 + 1) * U
# A filled pixel takes mean * 2 - 1: twice the mean's error and the last rounding.
FILL_TOL = 2 * MEAN_TOL + U


# ---------------------------------------------------------------------------------------------------------------------
# the statement
# ---------------------------------------------------------------------------------------------------------------------
def guidance_f64(geom):
    """(blur1 [K,R,R] float64, bg = blur1 > 0.99, n_bg [K], undecided) of geom [K,R,R] float32: ``default_gaussian_smoothing`` once
    (geom_metric.py:235), BG_THRESH (geom_metric.py:238-239)."""
    blur1 = br.blur_once(np.asarray(geom, np.float64))
    bg = blur1 > BG_THRESH
    return blur1, bg, bg.reshape(bg.shape[0], -1).sum(axis=1), np.abs(blur1 - BG_THRESH) <= UNDECIDED


def guidance_twice_0999_wrong(geom):
    """What ``nb_eval_masks_f32`` holds: two blurs and 0.999.  (Mutation reference.)"""
    blur = br.blur_twice(geom)
    bg = blur > 0.999
    return blur, bg, bg.reshape(bg.shape[0], -1).sum(axis=1), np.zeros_like(bg)


def on_white_f64(renders):
    """[n,3,R,R]: alpha * rgb + (1 - alpha) * 1.0 (geom_metric.py:197-198, 232-233)."""
    r = np.asarray(renders, np.float64)
    return r[:, 3:4] * r[:, :3] + (1 - r[:, 3:4])


def mean_colors_f64(renders, bg):
    """[n,3]: sum of the on-white colour over the background of drawing i % K, over max(count, 1) (geom_metric.py:239-241)."""
    n, k = renders.shape[0], bg.shape[0]
    m = bg[np.arange(n) % k][:, None].astype(np.float64)
    return (on_white_f64(renders) * m).sum(axis=(2, 3)) / np.clip(m.sum(axis=(2, 3)), 1.0, None)


def pairs_f64(renders, blur1, bg_of, mean, off0, off1, src1, p, transpose=True, masked=True, wrong=None):
    """(x [2n,3,p,p] float64, filled [n,p,p] bool) -- the LPIPS input of n pairs (geom_metric.py:244-259).  ``bg_of(values)`` decides
    background from blurred-guidance values (so that the wrong guidance brings its own threshold).  ``wrong``: None, or one of
    'no_transpose' (line 250 left out), 'fill_from_src' (the fill colour of image src1[i] instead of i, against lines 256-257),
    'mask_one_patch' (the first patch's mask only, against line 255)."""
    n, k = renders.shape[0], blur1.shape[0]
    rgb = on_white_f64(renders)
    src = np.arange(n) if src1 is None else np.asarray(src1)
    x0, x1, filled = np.zeros((n, 3, p, p)), np.zeros((n, 3, p, p)), np.zeros((n, p, p), bool)
    for i in range(n):
        j = int(src[i])
        (a, b), (c, d) = off0[i], off1[i]
        p0, g0 = rgb[i, :, a:a + p, b:b + p], blur1[i % k, a:a + p, b:b + p]
        p1, g1 = rgb[j, :, c:c + p, d:d + p], blur1[j % k, c:c + p, d:d + p]
        if transpose and wrong != "no_transpose":
            p1, g1 = p1.transpose(0, 2, 1), g1.T
        if masked:
            keep = bg_of(g0) if wrong == "mask_one_patch" else np.logical_and(bg_of(g0), bg_of(g1))
            mc = mean[j if wrong == "fill_from_src" else i][:, None, None]
            p0, p1 = np.where(keep[None], p0, mc), np.where(keep[None], p1, mc)
            filled[i] = ~keep
        x0[i], x1[i] = p0 * 2 - 1, p1 * 2 - 1
    return np.concatenate([x0, x1]), filled


def statement(c, wrong=None):
    """Everything of a pair case in float64: dict(blur1, bg, n_bg, und, mean, x, filled, und_pix [n,p,p])."""
    g = br.geom_f32(c["geom_u8"])
    blur1, bg, n_bg, und = guidance_twice_0999_wrong(g) if wrong == "twice_0999" else guidance_f64(g)
    thresh = 0.999 if wrong == "twice_0999" else BG_THRESH
    mean = mean_colors_f64(c["renders"], bg)
    x, filled = pairs_f64(c["renders"], blur1, lambda v: v > thresh, mean, c["off0"], c["off1"], c["src1"], c["p"], c["transpose"], c["masked"],
                          None if wrong == "twice_0999" else wrong)
    # a pair's pixel is undecided where either patch's guidance is
    und_pix = np.zeros_like(filled)
    if c["masked"]:
        n, k, p = filled.shape[0], und.shape[0], c["p"]
        src = np.arange(n) if c["src1"] is None else c["src1"]
        for i in range(n):
            (a, b), (cc, d), j = c["off0"][i], c["off1"][i], int(src[i])
            u1 = und[j % k, cc:cc + p, d:d + p]
            und_pix[i] = und[i % k, a:a + p, b:b + p] | (u1.T if c["transpose"] else u1)
    return dict(blur1=blur1, bg=bg, n_bg=n_bg, und=und, mean=mean, x=x, filled=filled, und_pix=und_pix)


WRONG = ("no_transpose", "fill_from_src", "mask_one_patch", "twice_0999")


# ---------------------------------------------------------------------------------------------------------------------
# checks shared by the CPU and the GPU test
# ---------------------------------------------------------------------------------------------------------------------
def check_guidance(blur1, n_bg, geom, what=""):
    """The blur within BLUR1_TOL of float64; at most 0.1 % of a drawing undecided; the count equal to the float64 one up to the
    undecided pixels, and equal to what the produced blur holds above 0.99f."""
    b64, bg, nb, und = guidance_f64(geom)
    k = geom.shape[0]
    assert np.abs(np.asarray(blur1, np.float64) - b64).max() <= BLUR1_TOL, (what, np.abs(blur1 - b64).max())
    assert np.all(und.reshape(k, -1).mean(axis=1) <= UNDECIDED_CAP), what
    assert np.array_equal((np.asarray(blur1) > np.float32(BG_THRESH))[~und], bg[~und]), what
    assert np.array_equal(np.asarray(n_bg), (np.asarray(blur1) > np.float32(BG_THRESH)).reshape(k, -1).sum(axis=1)), what
    assert np.all(np.abs(np.asarray(n_bg) - nb) <= und.reshape(k, -1).sum(axis=1)), what


def check_mean(mean, ref, what=""):
    """Within MEAN_TOL relative to the value.  The drawings of the cases leave no pixel undecided (asserted on the CPU), which this
    check relies on: an undecided pixel would move the sum by a whole colour."""
    assert not ref["und"].any(), what
    err = np.abs(np.asarray(mean, np.float64) - ref["mean"])
    assert np.all(err <= MEAN_TOL * np.abs(ref["mean"])), (what, float(err.max()))
    return float(err.max())


def check_pairs(x, ref, what=""):
    """Pixels that keep their colour within PIXEL_TOL, filled pixels within FILL_TOL, undecided pixels (at most 0.1 %) either."""
    n = ref["filled"].shape[0]
    und = np.concatenate([ref["und_pix"], ref["und_pix"]])[:, None]
    assert und.mean() <= UNDECIDED_CAP, what
    fill = np.concatenate([ref["filled"], ref["filled"]])[:, None]
    err = np.abs(np.asarray(x, np.float64) - ref["x"])
    tol = np.where(fill, FILL_TOL, PIXEL_TOL) * np.ones_like(err)
    bad = (err > tol) & ~und
    assert x.shape == ref["x"].shape and x.shape[0] == 2 * n and not bad.any(), (what, float(err[~np.broadcast_to(und, err.shape)].max()), int(bad.sum()))
    return float(err.max())


# ---------------------------------------------------------------------------------------------------------------------
# the cases: drawings, renders of brush_metrics_refs.cases(), and a plan
# ---------------------------------------------------------------------------------------------------------------------
def pair_cases():
    """[dict(name, geom_u8 [K,r,r], renders [n,4,r,r], p, transpose, masked, off0 [n,2], off1 [n,2], src1 [n] or None)]."""
    base = {c["name"]: c for c in br.cases()}
    out = []

    def add(name, of, p, transpose=True, masked=True, seed=0, src="perm", extremes=False, off=None):
        c = base[of]
        n, r = c["renders"].shape[0], c["geom_u8"].shape[-1]
        rs = np.random.RandomState(1000 + seed)
        off0, off1 = (rs.randint(0, r - p + 1, (n, 2)).astype(np.int32) for _ in range(2))
        if extremes:                                                      # both extreme offsets, and two different ones in one launch
            off0[0], off1[0], off0[1], off1[1] = (0, r - p), (r - p, 0), (r - p, r - p), (0, 0)
        if off is not None:
            off0[:len(off[0])], off1[:len(off[1])] = off
        if p == r:
            assert not off0.any() and not off1.any()
        src1 = {"perm": rs.permutation(n).astype(np.int32), "none": None, "shift": ((np.arange(n) + 3) % n).astype(np.int32)}[src]
        out.append(dict(name=name, geom_u8=c["geom_u8"], renders=c["renders"], p=p, transpose=transpose, masked=masked, off0=off0, off1=off1, src1=src1))

    add("r8_n300_k5_p6", "r8_n300_k5", 6, seed=1)                           # more workgroups than CUs, i % K wrapping
    add("r20_n7_k5_p16", "r20_n7_k5_values", 16, seed=2, src="none", extremes=True)
    add("r20_n7_k5_p7", "r20_n7_k5_values", 7, seed=3, extremes=True)       # odd p
    add("r33_n7_k5_p26", "r33_n7_k5", 26, seed=4, src="shift", extremes=True)             # i -> i + 3: another drawing (K = 5)
    add("r33_n7_k5_p33_across", "r33_n7_k5", 33, transpose=False, masked=False, seed=5)   # compute_lpips_across_geo's form
    add("r33_n7_k5_p33_transposed", "r33_n7_k5", 33, masked=False, seed=6)  # two LDS tiles per side, the second partial
    add("r20_n5_k1_all_stroke", "r20_n5_k1_no_background", 16, seed=7)      # no background: denominator 1, everything filled
    add("r20_n1_k1_all_background", "r20_n1_k1_no_foreground", 16, seed=8, src="none")
    # the vector path, whole LDS tiles: window columns that are multiples of four (16-byte loads) and that are not, in one launch
    add("r128_n2_k5_p64", "r128_n2_k5_calibration", 64, seed=9, off=([(0, 4), (13, 64)], [(64, 7), (8, 32)]))
    add("r128_n2_k5_p64_plain", "r128_n2_k5_calibration", 64, transpose=False, seed=10, src="none", off=([(3, 0), (1, 1)], [(0, 8), (2, 2)]))
    return out


def to_torch(c, device="cpu"):
    """(renders, geom [K,r,r] float32, off0, off1, src1) of a pair case as tensors."""
    t = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(device)
    return (t(c["renders"], torch.float32), t(br.geom_f32(c["geom_u8"]), torch.float32), t(c["off0"], torch.int32), t(c["off1"], torch.int32),
            t(c["src1"], torch.int32))


# ---------------------------------------------------------------------------------------------------------------------
# pair_distance: slim networks on pairs made from seeded renders
# ---------------------------------------------------------------------------------------------------------------------
# (arch: side of the renders, K drawings, n renders, seed).  p = default_patch_width(r): 64 at r = 128 (r // 2), 32 at r = 40 (0.8 r).
# The drawings are isolated dots and the renders dense noise (dotted_drawing has the reason); seeds: the first for which
# ``kink_margins`` holds with room for BOTH images of every pair and no pixel is undecided, found on the CPU with the float32
# restatement (tests/test_metric_patches_cpu.py asserts the margins again) -- alex, 8 images of 64 x 64: seed 3, smallest
# |pre-activation| 1312 and pool gap 92 float32-route errors (seeds 0 and 2 hold too, with 83 and 71 for the gap).  vgg, 4 images of
# 32 x 32 through lpips_refs.SLIM["vgg"]'s weights, which were normalised on tanh(randn) images: mostly opaque renders (alpha_lo) keep
# a like spread; of the seeds below 350 only 308 (187, 69), 322 (119, 73) and 349 (331, 88) hold, 349 with the most room.
# On the pairs the kernel makes (they differ from the restatement's in the last bits of the mean colour) one MI355X gave alex 1312 and
# 92, vgg 310 and 82.
DISTANCE_CASES = {"alex": dict(r=128, p=64, k=2, n=4, dots=8, alpha_lo=0, seed=3), "vgg": dict(r=40, p=32, k=2, n=2, dots=1, alpha_lo=192, seed=349)}


def dotted_drawing(rs, r, dots=8):
    """[r,r] uint8: background with a few single stroke pixels.  A dot takes the once-blurred guidance below 0.99 on the 21 pixels
    of a 5 x 5 block without its corners, and the zero padding does on the two pixels along every border: fill regions far smaller
    than what a pool window of either trunk sees, so no two of its inputs are equal by construction."""
    g = np.full((r, r), 255, np.uint8)
    g[rs.randint(0, r, dots), rs.randint(0, r, dots)] = 0
    return g


def distance_case(arch):
    """A pair case (masked, transposed, permuted) for ``pair_distance`` and the slim weights of lpips_refs.SLIM[arch]."""
    d = DISTANCE_CASES[arch]
    rs = np.random.RandomState(500 + d["seed"])
    geom = np.stack([dotted_drawing(rs, d["r"], d["dots"]) for _ in range(d["k"])])
    # (dense noise in all four planes: the renders of brush_metrics_refs.cases() have a fully clear quarter, constant white on white)
    ren = rs.randint(0, 256, (d["n"], 4, d["r"], d["r"]))
    ren[:, 3] = d["alpha_lo"] + ren[:, 3] % (256 - d["alpha_lo"])          # (alpha_lo: a mostly opaque render keeps the spread of its colours)
    ren = ren.astype(np.uint8).astype(np.float32) / np.float32(255)
    lim = d["r"] - d["p"]
    c = dict(name=f"distance_{arch}", geom_u8=geom, renders=ren, p=d["p"], transpose=True, masked=True,
             off0=rs.randint(0, lim + 1, (d["n"], 2)).astype(np.int32), off1=rs.randint(0, lim + 1, (d["n"], 2)).astype(np.int32),
             src1=rs.permutation(d["n"]).astype(np.int32))
    s = lr.SLIM[arch]
    return c, lr.slim_weights(arch, s["channels"], s["seed"], s["size"])


def pair_margins(weights, x):
    """``lpips_refs.kink_margins`` over BOTH images of every pair of x [2n,3,p,p] float32 (the forward value depends on the ReLU
    decisions of either): (smallest |pre-activation|, smallest pool gap, largest float32 error)."""
    n = x.shape[0] // 2
    out = []
    for a, b in ((x[:n], x[n:]), (x[n:], x[:n])):
        rec64, rec32 = [], []
        lr.lpips_f64(weights, a, torch.from_numpy(np.asarray(b)), record=rec64)
        lr.lpips_f64(weights, a, torch.from_numpy(np.asarray(b)), dtype=torch.float32, record=rec32)
        out.append(lr.kink_margins(rec64, rec32))
    return min(o[0] for o in out), min(o[1] for o in out), max(o[2] for o in out)


def distance_f64(weights, x):
    """[n] float64: LPIPS(x[i], x[n + i]) of x [2n,3,p,p] (any float dtype; taken as it is)."""
    n = x.shape[0] // 2
    return lr.lpips_f64(weights, np.asarray(x[:n], np.float64), np.asarray(x[n:], np.float64)).numpy()


# ---------------------------------------------------------------------------------------------------------------------
# the evaluator: the statement on the renders its passes produced
# ---------------------------------------------------------------------------------------------------------------------
def unit_scores(weights, geom_u8, renders, own, units, rounds, plan, p, pairs=None, dist=None):
    """{key: [nu]} of one pass: renders / own [nu*K,4,R,R], brush-major; ``plan`` = metrics.default_crops(...).  ``pairs(c)`` makes
    x of a pair case (default: the float64 statement), ``dist(x)`` the distances (default: ``distance_f64``)."""
    k = geom_u8.shape[0]
    nu = len(units)
    pairs = (lambda c: statement(c)["x"]) if pairs is None else pairs
    dist = (lambda x: distance_f64(weights, x)) if dist is None else dist
    rep = lambda name: np.concatenate([np.repeat(plan[name][b, j][None], k, 0) for b, j in units]).astype(np.int32)
    src = lambda name: np.concatenate([u * k + plan[name][b, j] for u, (b, j) in enumerate(units)]).astype(np.int32)
    base = dict(geom_u8=geom_u8, p=p, transpose=True, masked=True)
    multi = dict(base, renders=renders, off0=rep("multi_off0"), off1=rep("multi_off1"), src1=None)
    same = dict(base, renders=own, off0=rep("same_off0"), off1=rep("same_off1"), src1=src("same_perm"))
    zero = np.zeros((nu * k, 2), np.int32)
    geo = dict(geom_u8=geom_u8, renders=own, p=geom_u8.shape[-1], transpose=False, masked=False, off0=zero, off1=zero, src1=src("geo_perm"))
    val = lambda c: np.asarray(dist(pairs(c)), np.float64).reshape(nu, k).mean(axis=1)
    return {"LPIPS_UNIFORM_BG_multicolor": val(multi), "LPIPS_UNIFORM_BG": val(same), "LPIPS_ACROSS_GEO": val(geo)}


def scores_from_passes(weights, geom_u8, seen, n_brushes, rounds, plan, p, **how):
    """{key: [B]}: the mean over the rounds of ``unit_scores`` on what ``on_pass`` saw: [(units, renders, own_renders)]."""
    acc = {}
    for units, ren, own in seen:
        s = unit_scores(weights, geom_u8, ren, own, units, rounds, plan, p, **how)
        for key, v in s.items():
            for u, (b, _) in enumerate(units):
                acc.setdefault(key, {}).setdefault(b, []).append(v[u])
    assert all(sorted(per) == list(range(n_brushes)) and all(len(v) == rounds for v in per.values()) for per in acc.values())
    return {key: np.array([np.mean(per[b]) for b in range(n_brushes)]) for key, per in acc.items()}
