"""A float64 numpy statement of the brush scores and of their evaluation masks, and the shared cases (TEST ONLY): the torch routes'
test on the CPU, the kernels' test on the GPU and tests/golden/make_golden_brush_metrics.py are all held to the same inputs, rebuilt
from ``numpy.random.RandomState`` seeds.  Renders are ``uint8 / 255`` (plus a few hand-placed float32 values), so every input is exact
in float32.  The reference cannot run in float64 (its matrices are float32), so this statement is the project's own; the CPU test
holds it to what the reference returned (tests/golden/brush_metrics.npz)."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BG_THRESH, FG_THRESH = 0.999, 0.3
UNDECIDED = 1e-5                      # a pixel whose float64 blur lies this close to BG_THRESH may fall on either side in fp32
BLUR_TOL = 4e-6                       # two fp32 passes of <= 25 products and sums of values in 0..1: 2 * 26 * 2^-24 = 3.1e-6
CLARITY_TOL = 4e-6                    # exact inputs; only the fp32 summation errs
KERNEL_EPS_FACTOR = 4                 # the kernel may err by 4 * eps_ref per pixel (the device's fast exp2 / log2)


# ---------------------------------------------------------------------------------------------------------------------
# the statement
# ---------------------------------------------------------------------------------------------------------------------
def gauss5():
    g = np.exp(-0.5 * (np.arange(5, dtype=np.float64) - 2) ** 2)
    k = np.outer(g, g)
    return k / k.sum()


def blur_once(img):
    """[K,R,R] float64 -> the 5x5 Gaussian with zero padding 2."""
    k, r = img.shape[0], img.shape[1]
    p = np.zeros((k, r + 4, r + 4))
    p[:, 2:-2, 2:-2] = img
    w, out = gauss5(), np.zeros((k, r, r))
    for dy in range(5):
        for dx in range(5):
            out += w[dy, dx] * p[:, dy:dy + r, dx:dx + r]
    return out


def blur_twice(geom):
    return blur_once(blur_once(np.asarray(geom, np.float64)))


def blur_9x9_wrong(geom):
    """What a kernel that blurs a haloed tile twice WITHOUT re-zeroing computes: the first pass also fills the two pixels around
    the image.  (Mutation reference: the tests assert that the cases tell the two apart.)"""
    g = np.asarray(geom, np.float64)
    k, r = g.shape[0], g.shape[1]
    p = np.zeros((k, r + 4, r + 4))
    p[:, 2:-2, 2:-2] = g
    return blur_once(blur_once(p))[:, 2:-2, 2:-2]


def masks_f64(geom):
    """(blur, bg, fg, undecided) of geom [K,R,R] float32."""
    blur = blur_twice(geom)
    return blur, blur > BG_THRESH, np.asarray(geom, np.float32) < np.float32(FG_THRESH), np.abs(blur - BG_THRESH) <= UNDECIDED


def lab_f64(rgb):
    """[..., 3] sRGB in 0..1 -> CIE Lab, the constants of forger/util/color.py."""
    rgb = np.asarray(rgb, np.float64)
    with np.errstate(invalid="ignore"):
        lin = np.where(rgb <= 0.04045, rgb / 12.92, ((rgb + 0.055) / 1.055) ** 2.4)
    m = np.array([[0.412453, 0.212671, 0.019334], [0.357580, 0.715160, 0.119193], [0.180423, 0.072169, 0.950227]])
    xyz = (lin @ m) * np.array([1 / 0.95047, 1.0, 1 / 1.08883])
    d = 6.0 / 29.0
    with np.errstate(invalid="ignore"):
        f = np.where(xyz < d ** 3, xyz / (3 * d * d) + 4.0 / 29, np.cbrt(xyz + 1e-8))
    return np.stack([116 * f[..., 1] - 16, 500 * (f[..., 0] - f[..., 1]), 200 * (f[..., 1] - f[..., 2])], axis=-1)


def deltas_f64(targets, renders, ignore_transparency=False):
    """[n,R,R]: Lab distance of every pixel of renders [n,4,R,R] to targets [n,3]."""
    r = np.asarray(renders, np.float64)
    rgb = r[:, :3] if ignore_transparency else r[:, 3:4] * r[:, :3] + (1 - r[:, 3:4])
    lab = lab_f64(np.moveaxis(rgb, 1, -1))
    return np.sqrt(((lab - lab_f64(np.asarray(targets, np.float64))[:, None, None, :]) ** 2).sum(axis=-1))


def image_sums_f64(deltas, geom, k, lab_thresh):
    """Per image i on drawing i % k: (sum w dE, sum w [dE > t], sum w)."""
    n = deltas.shape[0]
    w = 1 - np.asarray(geom, np.float64)[np.arange(n) % k]
    return (w * deltas).sum(axis=(1, 2)), (w * (deltas > lab_thresh)).sum(axis=(1, 2)), w.sum(axis=(1, 2))


def lab_metrics_f64(targets, renders, geom, lab_thresh=10, ignore_transparency=False, deltas=None):
    """(LAB_E%, LAB_L2) per image [n]; the reference's value is their mean over the batch."""
    d = deltas_f64(targets, renders, ignore_transparency) if deltas is None else deltas
    s_de, s_e, s_w = image_sums_f64(d, geom, np.asarray(geom).shape[0], lab_thresh)
    return s_e / np.clip(s_w, 1, None) * 100, s_de / (d.shape[1] * d.shape[2])


def transparency_f64(renders, bg, fg):
    """(BG_CLARITY_MEAN, FG_OPACITY_MEDIAN) of renders [n,4,R,R] pooled; image i uses mask i % K.  The mean in float64; the median
    the LOWER median of a numpy sort of the float32 alphas, no arithmetic.  NaN where the selection is empty."""
    n, k = renders.shape[0], bg.shape[0]
    idx = np.arange(n) % k
    alpha = np.asarray(renders)[:, 3]
    a_bg, a_fg = alpha[bg[idx]], np.sort(alpha[fg[idx]].astype(np.float32), kind="stable")
    clarity = 1 - a_bg.astype(np.float64).mean() if a_bg.size else np.nan
    return clarity, (a_fg[(a_fg.size - 1) // 2] if a_fg.size else np.float32(np.nan))


def brush_scores_f64(renders, targets, geom, lab_thresh=10, skip=None):
    """The four scores [nb] of renders [nb*K,4,R,R], brush-major, as BrushEvaluator states them; plus, for LAB_E%, the values at
    thresholds lab_thresh -+ skip (a pair of arrays) when ``skip`` is given."""
    k = np.asarray(geom).shape[0]
    nb = renders.shape[0] // k
    _, bg, fg, _ = masks_f64(geom)
    d = deltas_f64(targets, renders)
    e, l2 = lab_metrics_f64(targets, renders, geom, lab_thresh, deltas=d)
    out = {"LAB_E%": e.reshape(nb, k).mean(axis=1), "LAB_L2": l2.reshape(nb, k).mean(axis=1)}
    tr = [transparency_f64(renders[b * k:(b + 1) * k], bg, fg) for b in range(nb)]
    out["BG_CLARITY_MEAN"] = np.array([t[0] for t in tr])
    out["FG_OPACITY_MEDIAN"] = np.array([t[1] for t in tr], np.float32)
    if skip is not None:
        out["LAB_E%_band"] = tuple(lab_metrics_f64(targets, renders, geom, lab_thresh + s, deltas=d)[0].reshape(nb, k).mean(axis=1)
                                   for s in (skip, -skip))                 # (a higher threshold counts fewer pixels: the lower end first)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# tolerances, from eps_ref (the reference's own float32 evaluation against this statement, stored in the fixture)
# ---------------------------------------------------------------------------------------------------------------------
def check_scores(got, want, eps, what=""):
    """``got``: {key: [nb] float32}; ``want``: brush_scores_f64(..., skip=KERNEL_EPS_FACTOR * eps).  LAB_L2 within 4 eps + 1e-5 |v|;
    LAB_E% between the float64 values at thresholds -+ 4 eps (and the 1e-5 |v| of the fp32 sums and quotient, as for LAB_L2: without
    it the band is a single float64 number whenever no pixel lies that close to the threshold); the clarity within 4e-6; the median
    bit for bit."""
    tol = KERNEL_EPS_FACTOR * eps
    g = {k: np.asarray(v) for k, v in got.items()}
    l2 = want["LAB_L2"]
    assert np.all(np.abs(g["LAB_L2"] - l2) <= tol + 1e-5 * np.abs(l2)), (what, g["LAB_L2"], l2)
    lo, hi = want["LAB_E%_band"]
    assert np.all(g["LAB_E%"] >= lo - 1e-5 * np.abs(lo)) and np.all(g["LAB_E%"] <= hi + 1e-5 * np.abs(hi)), (what, g["LAB_E%"], lo, hi)
    c = want["BG_CLARITY_MEAN"]
    assert np.array_equal(np.isnan(g["BG_CLARITY_MEAN"]), np.isnan(c)), (what, g["BG_CLARITY_MEAN"], c)
    assert np.all(np.abs(g["BG_CLARITY_MEAN"] - c)[~np.isnan(c)] <= CLARITY_TOL), (what, g["BG_CLARITY_MEAN"], c)
    assert np.array_equal(g["FG_OPACITY_MEDIAN"].astype(np.float32), want["FG_OPACITY_MEDIAN"], equal_nan=True), \
        (what, g["FG_OPACITY_MEDIAN"], want["FG_OPACITY_MEDIAN"])


def check_masks(blur, mask, n_bg, n_fg, geom, what=""):
    """The blur within BLUR_TOL of float64; the mask bits equal to the float64 ones except on undecided pixels (at most 0.1 % per
    drawing); the counts equal to the produced mask's."""
    b64, bg, fg, und = masks_f64(geom)
    assert np.abs(blur.astype(np.float64) - b64).max() <= BLUR_TOL, (what, np.abs(blur - b64).max())
    k = geom.shape[0]
    assert np.all(und.reshape(k, -1).mean(axis=1) <= 1e-3), what
    assert np.array_equal((mask & 1).astype(bool)[~und], bg[~und]), what
    assert np.array_equal((mask >> 1).astype(bool), fg) and mask.max() <= 3, what
    assert np.array_equal(n_bg, (mask & 1).reshape(k, -1).sum(axis=1)) and np.array_equal(n_fg, (mask >> 1).reshape(k, -1).sum(axis=1)), what


# ---------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------
def smooth_drawing(rs, r, lines=2):
    """An anti-aliased drawing [r,r] uint8: a few soft lines, so that w = 1 - geom takes values between 0 and 1."""
    yy, xx = np.mgrid[0:r, 0:r].astype(np.float64)
    d = np.full((r, r), 1e9)
    for _ in range(lines):
        a, c = rs.uniform(0, np.pi), rs.uniform(0.2, 0.8, 2) * r
        d = np.minimum(d, np.abs((xx - c[0]) * np.sin(a) - (yy - c[1]) * np.cos(a)))
    return np.clip((d - max(0.8, r / 24)) * (255 / 1.5), 0, 255).astype(np.uint8)


def border_drawing(r):
    """Binary strokes that touch every border and all four corners: where the zero padding between the two blurs shows."""
    g = np.full((r, r), 255, np.uint8)
    t = max(1, r // 10)
    g[:t, :r // 2] = 0
    g[r - t:, r // 3:] = 0
    g[r // 4:, :t] = 0
    g[:r // 2, r - t:] = 0
    for y, x in ((0, 0), (0, r - 2), (r - 2, 0), (r - 2, r - 2)):
        g[y:y + 2, x:x + 2] = 0
    return g


def cal_drawings():
    with np.load(os.path.join(GOLDEN, "engine_r128.npz")) as z:
        return z["uvs_cal_medium"].copy()


def _renders(rs, n, r):
    """[n,4,r,r] float32 = uint8 / 255, with fully clear and fully opaque regions."""
    u = rs.randint(0, 256, (n, 4, r, r)).astype(np.uint8)
    u[:, 3, : max(1, r // 4)] = 0                                          # alpha 0
    u[:, 3, r - max(1, r // 4):] = 255                                     # alpha 1
    return u.astype(np.float32) / np.float32(255)


def _special_values(ren):
    """Into the opaque last rows of image 0: channels at 0, at 0.04045 and the next float up, near black (f() takes its linear
    branch), and white."""
    up = np.nextafter(np.float32(0.04045), np.float32(1))
    vals = np.array([[0, 0, 0], [0.04045, 0.04045, 0.04045], [up, up, up], [0.04045, up, 0], [0.01, 0.02, 0.005], [0.003, 0, 0.001],
                     [1, 1, 1], [1, 0, 0.04045]], np.float32)
    r = ren.shape[-1]
    for j, v in enumerate(vals):
        ren[0, :3, r - 1, j % r] = v
        ren[0, 3, r - 1, j % r] = 1
    return ren


def cases():
    """[dict(name, geom_u8 [K,r,r], renders [n,4,r,r] float32, targets [n,3] float32, lab_thresh, ignore)]: R in {8, 20, 33, 128}, n in
    {1, 5, 7, 300}, K in {1, 5}."""
    out = []

    def add(name, seed, geom_u8, n, ignore=False, lab_thresh=10, special=False, targets=None):
        rs = np.random.RandomState(seed)
        r = geom_u8.shape[-1]
        ren = _renders(rs, n, r)
        tg = (rs.randint(0, 256, (n, 3)).astype(np.uint8).astype(np.float32) / np.float32(255))
        if special:
            ren = _special_values(ren)
        if targets is not None:
            tg[:len(targets)] = np.asarray(targets, np.float32)
        out.append(dict(name=name, geom_u8=np.ascontiguousarray(geom_u8), renders=ren, targets=tg, lab_thresh=lab_thresh, ignore=ignore))

    rs = np.random.RandomState(100)
    five8 = np.stack([smooth_drawing(rs, 8, 1) for _ in range(5)])
    five20 = np.stack([smooth_drawing(rs, 20), border_drawing(20), smooth_drawing(rs, 20), smooth_drawing(rs, 20, 3), smooth_drawing(rs, 20)])
    # (drawn from the stream of seed 100, the third of these had two pixels 3e-8 from the background threshold: its own seed instead;
    # tests/test_brush_metrics_cpu.py checks that no drawing of the cases leaves a pixel undecided)
    five33 = np.stack([border_drawing(33), smooth_drawing(rs, 33), smooth_drawing(np.random.RandomState(133), 33, 3), smooth_drawing(rs, 33),
                       smooth_drawing(rs, 33)])
    add("r8_n300_k5", 1, five8, 300)                                        # more workgroups than CUs, i % K wrapping
    add("r20_n7_k5_values", 2, five20, 7, special=True, targets=[[1, 1, 1], [0, 0, 0]])
    add("r20_n5_k5_ignore", 3, five20, 5, ignore=True, targets=[[0, 0, 0], [1, 1, 1]], lab_thresh=25)
    add("r33_n7_k5", 4, five33, 7, special=True)
    add("r33_n5_k1_border_ignore", 5, five33[:1], 5, ignore=True, lab_thresh=40)
    add("r20_n1_k1_no_foreground", 6, np.full((1, 20, 20), 255, np.uint8), 1)
    add("r20_n5_k1_no_background", 7, np.zeros((1, 20, 20), np.uint8), 5)
    add("r128_n2_k5_calibration", 8, cal_drawings(), 2, targets=[[1, 1, 1]])
    add("r128_n1_k1", 9, cal_drawings()[3:4], 1, lab_thresh=60)
    return out


def geom_f32(geom_u8):
    return geom_u8.astype(np.float32) / np.float32(255)


def mask_drawings():
    """{name: [K,r,r] uint8}: every distinct set of drawings of the cases."""
    return {c["name"]: c["geom_u8"] for c in cases()}


EVAL_SEED, EVAL_ROUNDS = 0, 2          # the evaluator's default colour stream stored in the fixture: 4 brushes x 2 rounds x (5, 3)


# ---------------------------------------------------------------------------------------------------------------------
# checks shared by the CPU and the GPU test
# ---------------------------------------------------------------------------------------------------------------------
def _expand(c):
    """(geom [K,r,r] float32, geom per image [n,1,r,r]) of a case."""
    g = geom_f32(c["geom_u8"])
    n = c["renders"].shape[0]
    return g, g[np.arange(n) % g.shape[0]][:, None]


def _pooled_f64(c, skip):
    """The reference's four scalars of a case in float64: all n images of the case as ONE batch."""
    g, _ = _expand(c)
    _, bg, fg, _ = masks_f64(g)
    d = deltas_f64(c["targets"], c["renders"], c["ignore"])
    e, l2 = lab_metrics_f64(c["targets"], c["renders"], g, c["lab_thresh"], deltas=d)
    lo = lab_metrics_f64(c["targets"], c["renders"], g, c["lab_thresh"] + skip, deltas=d)[0]
    hi = lab_metrics_f64(c["targets"], c["renders"], g, c["lab_thresh"] - skip, deltas=d)[0]
    cl, med = transparency_f64(c["renders"], bg, fg)
    return {"LAB_E%": np.array([e.mean()]), "LAB_L2": np.array([l2.mean()]), "BG_CLARITY_MEAN": np.array([cl]),
            "FG_OPACITY_MEDIAN": np.array([med], np.float32), "LAB_E%_band": (np.array([lo.mean()]), np.array([hi.mean()]))}


def check_image_sums(sums, c, d64, eps):
    """The four per-image sums of ``brush_metrics`` against float64, in the units of the metrics they feed."""
    g, _ = _expand(c)
    n, k, count = sums.shape[0], g.shape[0], g.shape[1] * g.shape[2]
    tol = KERNEL_EPS_FACTOR * eps
    s_de, s_e, s_w = image_sums_f64(d64, g, k, c["lab_thresh"])
    l2 = s_de / count
    assert np.all(np.abs(sums[:, 0] / count - l2) <= tol + 1e-5 * np.abs(l2)), c["name"]
    assert np.all(np.abs(sums[:, 2] - s_w) <= 1e-5 * np.abs(s_w) + 1e-6), c["name"]
    lo = image_sums_f64(d64, g, k, c["lab_thresh"] + tol)[1]
    hi = image_sums_f64(d64, g, k, c["lab_thresh"] - tol)[1]
    assert np.all(sums[:, 1] >= lo - 1e-5 * lo) and np.all(sums[:, 1] <= hi + 1e-5 * hi), c["name"]
    _, bg, _, _ = masks_f64(g)
    idx = np.arange(n) % k
    want = np.array([c["renders"][i, 3][bg[idx[i]]].astype(np.float64).sum() for i in range(n)])
    nb = np.maximum(bg.reshape(k, -1).sum(axis=1)[idx], 1)
    assert np.all(np.abs(sums[:, 3] - want) / nb <= CLARITY_TOL), c["name"]


def scores_from_passes(seen, geom_u8, n_brushes, rounds, eps, lab_thresh=10):
    """The float64 statement on the renders the passes produced: {key: [B]} means over the rounds, with the LAB_E% band."""
    g = geom_f32(geom_u8)
    acc = {}
    for units, ren, tg in seen:
        s = brush_scores_f64(ren, tg, g, lab_thresh, skip=KERNEL_EPS_FACTOR * eps)
        for j, (b, r) in enumerate(units):
            for key, v in s.items():
                vals = [x[j] for x in v] if isinstance(v, tuple) else v[j]
                acc.setdefault(key, {}).setdefault(b, []).append(vals)
    out = {}
    for key, per in acc.items():
        assert sorted(per) == list(range(n_brushes)) and all(len(v) == rounds for v in per.values())
        if key == "LAB_E%_band":
            out[key] = tuple(np.array([np.mean([v[i] for v in per[b]]) for b in range(n_brushes)]) for i in range(2))
        elif key == "FG_OPACITY_MEDIAN":
            out[key] = np.array([np.mean(np.array(per[b], np.float32), dtype=np.float32) for b in range(n_brushes)], np.float32)
        else:
            out[key] = np.array([np.mean(per[b]) for b in range(n_brushes)])
    return out


def check_against_passes(scores, seen, geom_u8, rounds, eps):
    want = scores_from_passes(seen, geom_u8, len(scores.ids), rounds, eps)
    got = dict(scores.as_dict())
    if rounds > 1:                      # the mean of `rounds` float32 medians: one rounding of a sum of values in 0..1
        assert np.all(np.abs(got["FG_OPACITY_MEDIAN"] - want["FG_OPACITY_MEDIAN"]) <= 2.0 ** -23)
        got["FG_OPACITY_MEDIAN"] = want["FG_OPACITY_MEDIAN"]
    check_scores(got, want, eps, "evaluator")
