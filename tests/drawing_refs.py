"""Scenes and helpers of the synthetic-drawing tests (csrc/nb_drawings.hip): what tests/test_hip_drawings.py runs on the device and
tests/test_drawings_cpu.py holds to the scenes' conditions without one -- the band share of every raster scene
(``stroke_refs.BAND_CAP``) and the distance of every thickness try of the fixed seeds from a rounding or acceptance boundary."""
import numpy as np

import stroke_refs as sr
from brushstroke_engine_amd import drawings as dr

# ---------------------------------------------------------------------------------------------------------------------
# the sampler: K = 64 drawings, two sides, two placements, three thickness modes
# ---------------------------------------------------------------------------------------------------------------------
CTRL_K = 64
CTRL_SIDES = (64, 256)
CTRL_OFFSET = 7
HALF_MARGIN = 1e-3           # no evaluated thickness try of the fixed seeds has v this close to a half-integer (float64)
# fixed after tests/test_drawings_cpu.py::test_gpu_seeds_keep_clear_of_the_boundaries passed for each of them
CTRL_SEEDS = {64: 5, 256: 6}
E2E_R, E2E_K, E2E_SEED = 64, 8, 13


def ctrl_specs(r):
    """{name: SplineSpec}: both placements with each of the three thickness modes, thickness scaled to side r."""
    out = {}
    for mode in ("cells", "uniform"):
        base = dr.SplineSpec(mode=mode, pts_min=4, pts_max=20).scaled(r)          # (20 > 16: the cells mode's free placement too)
        out[f"{mode}-mixture"] = base
        out[f"{mode}-range"] = dr.SplineSpec(mode=mode, thick="range", rmin=1, rmax=6)
        out[f"{mode}-fixed"] = base.fixed(3)
    return out


def e2e_spec():
    return dr.SplineSpec(mode="cells").scaled(E2E_R)


def evaluated_tries(spec, seed, offset, k):
    """The values v of the Gaussian tries the kernel evaluates: every try of a drawing up to and including the first accepted one."""
    v = dr.thickness_tries_numpy(spec, seed, offset, k)
    ok = v >= -0.5
    last = np.where(ok.any(axis=1), np.argmax(ok, axis=1), v.shape[1] - 1)
    return v[np.arange(v.shape[1])[None, :] <= last[:, None]]


def half_distance(v):
    """Distance of every v to the nearest half-integer: the rounding boundaries of rintf and the acceptance boundary -0.5."""
    return np.abs(v - np.floor(v) - 0.5)


def cells_of(ctrl_rows, r):
    """Cell index (cy * 4 + cx) of control points in pixels of side r."""
    q = r / 4.0
    return (np.floor(ctrl_rows[:, 1] / q) * 4 + np.floor(ctrl_rows[:, 0] / q)).astype(np.int64)


def coord_bound(r):
    """NB_SYNTH_COORD_ROUNDINGS fp32 roundings (counted in the header comment of csrc/nb_drawings.hip), one ulp(1.1 r) each."""
    from brushstroke_engine_amd import _lib
    return _lib.NB_SYNTH_COORD_ROUNDINGS * float(np.spacing(np.float32(1.1 * r)))


# ---------------------------------------------------------------------------------------------------------------------
# the batch raster: fixed rows
# ---------------------------------------------------------------------------------------------------------------------
def _case(name, parts, h, w, off=(0, 0), lead=0, seg_off=None, exact=False):
    """parts: one [n, 8] float32 array per drawing, laid out one after the other."""
    segs = np.concatenate(parts) if parts else np.zeros((0, 8), np.float32)
    if seg_off is None:
        seg_off = np.concatenate([[0], np.cumsum([len(p) for p in parts])])
    return dict(name=name, segs=np.ascontiguousarray(segs, np.float32), seg_off=np.asarray(seg_off, np.int32), k=len(seg_off) - 1, h=h,
                w=w, off=off, lead=lead, exact=exact)


def clipping_parts(h, w):
    """Drawing 0: curves that leave through the bottom, right and top edges and the bottom right corner; drawing 1: nothing.  In
    memory drawing 1 follows drawing 0, so a row that is not clipped at the bottom edge would darken it."""
    rows = sr.rows8([(w / 2 + 0.25, h - 10.5, w / 2 + 3.25, h + 30.5, 3.0), (w - 6.5, h / 2, w + 20.5, h / 2 + 4.25, 2.5),
                     (w / 3, 8.5, w / 3 + 2.5, -25.0, 2.0), (w - 9.0, h - 7.0, w + 11.0, h + 13.0, 4.5), (w / 4, h + 1.25, w / 4, h + 1.25, 3.0)])
    return [rows, np.zeros((0, 8), np.float32)]


def batch_cases():
    e = np.zeros((0, 8), np.float32)
    rnd = lambda n, h, w, seed, **kw: sr.random_scene(n, h, w, seed=seed, **kw)          # noqa: E731
    cases = [
        _case("k3-64x64", [rnd(40, 64, 64, 1), rnd(3, 64, 64, 2), rnd(40, 64, 64, 3)], 64, 64),
        _case("k3-96x80-lead1", [rnd(40, 96, 80, 4), rnd(40, 96, 80, 5), rnd(300, 96, 80, 6, length=12.0, rmax=2.0)], 96, 80, lead=1),
        _case("k3-70x130-lead1+3-5", [rnd(40, 70, 130, 7), rnd(40, 70, 130, 8), rnd(40, 70, 130, 9)], 70, 130, off=(3, -5), lead=1),
        _case("k5-empties", [e, rnd(40, 63, 65, 10), e, rnd(40, 63, 65, 11), e], 63, 65, off=(3, -5)),
        _case("k2-dead-rows", [np.concatenate([sr.dead_rows()[:7], rnd(20, 63, 65, 12), sr.dead_rows()[7:]]), sr.dead_rows()], 63, 65),
        _case("k2-clipping", clipping_parts(70, 66), 70, 66),
        _case("k2-exact", [sr.exact_scene(130, 257)] * 2, 130, 257, off=(7, 13), exact=True),
    ]
    # ranges outside 0..n (120 rows): drawing 0 = rows 0..40; 1 = 40..-3 (decreasing); 2 = -3..80 (below 0); 3 = 80..200 (past the
    # end); 4 = 200..120 (decreasing, past the end); 5 = 120..120 (empty at the end); 6 = 120..2^31-1
    bad = _case("k7-bad-ranges", [rnd(120, 63, 65, 13)], 63, 65, seg_off=[0, 40, -3, 80, 200, 120, 120, 2 ** 31 - 1])
    cases.append(bad)
    return cases


def drawing_rows(case, i):
    """The rows drawing i of a batch case is made of: its range of segs, or none if the range is not inside the rows."""
    a, b = int(case["seg_off"][i]), int(case["seg_off"][i + 1])
    return case["segs"][a:b] if 0 <= a <= b <= len(case["segs"]) else case["segs"][:0]


_MARGINS = {}


def case_margin(case, i):
    """margin64 of drawing i of a batch case, computed once per process."""
    key = (case["name"], i)
    if key not in _MARGINS:
        _MARGINS[key] = sr.margin64(drawing_rows(case, i), case["h"], case["w"], case["off"])
    return _MARGINS[key]
