"""Golden samples of the reference's Catmull-Rom spline (forger/core/curve.py, ``CatmullRomSpline``): its knots ``ts`` and
``sample_t`` results for a handful of control sets.  Only the recorded numbers are committed (spline_samples.npz).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_spline.py

The reference computes in float32 (float32 control points and knots); the script prints how far the float64 restatement
(tests/stroke_refs.py) is from it, relative to each set's coordinate extent.  tests/test_stroke_refs_cpu.py notes that figure.
"""
import bisect
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.environ.get("FORGER_REFERENCE", "/root/reference"))
# curve.py imports skimage.draw only for `line` (draw_spline_lib); scikit-image is not installed here
sk, skd = types.ModuleType("skimage"), types.ModuleType("skimage.draw")
skd.line = lambda *a, **k: (_ for _ in ()).throw(RuntimeError("not available"))
sk.draw = skd
sys.modules.update({"skimage": sk, "skimage.draw": skd})
from forger.core.curve import CatmullRomSpline  # noqa: E402

import stroke_refs  # noqa: E402


def control_sets():
    rs = np.random.RandomState(20)
    sets = {
        "four": np.array([[10, 20], [60, 35], [110, 90], [150, 60]], np.float32),                       # the smallest spline
        "nine": (rs.rand(9, 2) * 240 + 8).astype(np.float32),
        "collinear": np.stack([np.linspace(5, 245, 6), np.linspace(30, 200, 6) + np.array([0, 1e-3, -2e-3, 1e-3, 0, 2e-3])], 1).astype(np.float32),
        "unequal": np.array([[12, 12], [12.5, 12.25], [200, 40], [201, 41], [201.5, 240], [30, 236]], np.float32),   # gaps 0.5 .. 200
        "unit": (rs.rand(7, 2) * 2 - 1).astype(np.float32),                                              # the reference's [-1, 1] range
    }
    return sets


def main():
    out = {}
    worst = 0.0
    for name, pts in control_sets().items():
        sp = CatmullRomSpline(pts, alpha=0.5)
        ts = np.asarray(sp.ts, np.float64)
        # parameters strictly inside (ts[1], ts[-2]]: sample_t's bisection is defined there
        fr = np.concatenate([np.linspace(0, 1, 23)[1:], [1e-3, 0.5, 0.999]])
        t = np.array([np.float32(ts[1] + f * (ts[-2] - ts[1])) for f in fr], np.float64)
        t = t[(t > ts[1]) & (t <= ts[-2])]
        idx = np.array([min(bisect.bisect_left(sp.ts, float(v)) - 2, pts.shape[0] - 4) for v in t], np.int32)
        got = np.stack([np.asarray(sp.sample_t(float(v)), np.float64) for v in t])
        want = np.stack([stroke_refs.sample(pts, v, int(i)) for v, i in zip(t, idx)])
        extent = float(np.ptp(pts, axis=0).max())
        dev = float(np.abs(got - want).max()) / extent
        ts_dev = float(np.abs(ts - stroke_refs.knots(pts)).max() / ts[-1])
        print(f"{name:10s} {len(t):3d} samples  extent {extent:8.3f}  max |reference - float64| / extent = {dev:.3e}   knots (relative) {ts_dev:.3e}")
        worst = max(worst, dev)
        out.update({f"{name}_ctrl": pts, f"{name}_ts": ts, f"{name}_t": t, f"{name}_idx": idx, f"{name}_pts": got})
    print(f"largest deviation relative to the extent: {worst:.3e}")
    out["names"] = np.array(sorted(control_sets()))
    out["max_rel_dev"] = np.float64(worst)
    np.savez(os.path.join(HERE, "spline_samples.npz"), **out)


if __name__ == "__main__":
    main()
