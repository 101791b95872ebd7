"""Vector strokes: polylines and centripetal Catmull-Rom splines as capsule segments (host side; nothing of ``tiling``, ``tile_ops`` or
``painting``).

``StrokeList`` holds strokes as points and radii, in the float32 values the device reads.  The numpy functions restate the two kernels of
``csrc/nb_strokes.hip`` -- ``nb_spline_flatten_f32`` and ``nb_raster_segments_u8`` -- in float64: they are what the tests hold the
kernels to, and what an ops without the kernels rasterises with (``TileOpsBase.raster_strokes``)."""
from __future__ import annotations

import json
from typing import List, Optional, Tuple

import numpy as np

from . import _lib

SEG_PITCH = _lib.NB_SEG_PITCH     # floats per segment row: x0, y0, x1, y1, r, three reserved


class StrokeList:
    """Strokes as points: what a tablet or a vector file gives, and what ``TileOps.raster_strokes`` /
    ``PaintingHelper.paint_strokes`` turn into the geometry without a raster on the host.

    Coordinates are drawing coordinates ``(x, y)`` in pixels; pixel (row y, column x) has its centre at exactly ``(x, y)``.
    A stroke covers every pixel whose centre is within the radius of its centre line.  Everything is kept as float32, the
    values the device reads.

    JSON schema (``to_json`` / ``from_json``): a list of objects
    ``{"type": "polyline" | "spline", "points": [[x, y], ...], "radius": r | [r, ...]}``; a spline may carry
    ``"through_ends": false`` (default true)."""

    def __init__(self):
        self.items: List[dict] = []           # what was added, in order (the JSON form)
        self._poly: List[np.ndarray] = []     # [n, 5] float32 segment rows per polyline
        self._ctrl: List[np.ndarray] = []     # [P, 3] float32 control points (x, y, r) per spline, phantom ends included

    @staticmethod
    def _points_radius(points, radius) -> Tuple[np.ndarray, np.ndarray]:
        p = np.asarray(points, np.float32)
        if p.ndim != 2 or p.shape[1] != 2 or p.shape[0] < 1:
            raise ValueError(f"stroke points must be [K, 2] with K >= 1, got {p.shape}")
        r = np.asarray(radius, np.float32)
        if r.ndim == 0:
            r = np.full(p.shape[0], r, np.float32)
        if r.shape != (p.shape[0],):
            raise ValueError(f"radius must be a scalar or one per point ({p.shape[0]}), got {r.shape}")
        if not (np.isfinite(p).all() and np.isfinite(r).all() and (r >= 0).all()):
            raise ValueError("stroke points and radii must be finite, radii >= 0")
        return p, r

    @staticmethod
    def _json_radius(radius):
        r = np.asarray(radius, np.float32)
        return float(r) if r.ndim == 0 else [float(v) for v in r]

    def add_polyline(self, points, radius) -> "StrokeList":
        """Straight segments through ``points`` [K, 2]; ``radius`` a scalar or one per point (a segment's radius is the mean of
        its end points').  A single point is a disc."""
        p, r = self._points_radius(points, radius)
        if p.shape[0] == 1:
            p, r = np.repeat(p, 2, 0), np.repeat(r, 2)
        rows = np.concatenate([p[:-1], p[1:], ((r[:-1] + r[1:]) * np.float32(0.5))[:, None]], axis=1).astype(np.float32)
        self._poly.append(rows)
        self.items.append({"type": "polyline", "points": np.asarray(points, np.float32).tolist(), "radius": self._json_radius(radius)})
        return self

    def add_spline(self, points, radius, through_ends: bool = True) -> "StrokeList":
        """A centripetal Catmull-Rom spline (the curve of the reference's ``forger/core/curve.py``) through ``points`` [K, 2];
        ``radius`` a scalar or one per point, interpolated linearly along each span.  The curve of P control points runs from the
        second to the last but one; ``through_ends`` adds the reflected phantom points ``2 P0 - P1`` and ``2 P_last - P_prev`` so
        that it passes through the first and last given point.  Consecutive duplicate points are dropped (a repeated control point
        has no curve: its knot interval is zero)."""
        p, r = self._points_radius(points, radius)
        keep = np.concatenate([[True], np.any(p[1:] != p[:-1], axis=1)])
        p, r = p[keep], r[keep]
        if through_ends:
            if p.shape[0] < 2:
                raise ValueError("a spline through its ends needs at least 2 distinct points")
            p = np.concatenate([(2 * p[:1] - p[1:2]), p, (2 * p[-1:] - p[-2:-1])]).astype(np.float32)
            r = np.concatenate([r[:1], r, r[-1:]])
        if p.shape[0] < 4:
            raise ValueError(f"a spline needs at least 4 distinct control points, got {p.shape[0]}")
        self._ctrl.append(np.concatenate([p, r[:, None]], axis=1).astype(np.float32))
        item = {"type": "spline", "points": np.asarray(points, np.float32).tolist(), "radius": self._json_radius(radius)}
        if not through_ends:
            item["through_ends"] = False
        self.items.append(item)
        return self

    def __len__(self) -> int:
        return len(self.items)

    def to_json(self) -> str:
        return json.dumps(self.items)

    @classmethod
    def from_json(cls, text) -> "StrokeList":
        """From a JSON string or the list it decodes to."""
        data = json.loads(text) if isinstance(text, (str, bytes)) else text
        if not isinstance(data, list):
            raise ValueError("strokes JSON: a list of stroke objects expected")
        out = cls()
        for it in data:
            kind = it.get("type") if isinstance(it, dict) else None
            if kind == "polyline":
                out.add_polyline(it["points"], it["radius"])
            elif kind == "spline":
                out.add_spline(it["points"], it["radius"], through_ends=bool(it.get("through_ends", True)))
            else:
                raise ValueError(f"strokes JSON: unknown stroke {it!r}")
        return out

    def polyline_segments(self) -> np.ndarray:
        """[n, SEG_PITCH] float32 segment rows of all polylines."""
        rows = np.zeros((sum(a.shape[0] for a in self._poly), SEG_PITCH), np.float32)
        if self._poly:
            rows[:, :5] = np.concatenate(self._poly)
        return rows

    def spline_control(self) -> Tuple[np.ndarray, np.ndarray]:
        """(ctrl [P_total, 3] float32, stroke_off [n_splines + 1] int32): the inputs of ``nb_spline_flatten_f32``."""
        off = np.zeros(len(self._ctrl) + 1, np.int32)
        np.cumsum([a.shape[0] for a in self._ctrl], out=off[1:])
        ctrl = np.concatenate(self._ctrl) if self._ctrl else np.zeros((0, 3), np.float32)
        return np.ascontiguousarray(ctrl, np.float32), off

    def spline_segment_count(self, subdiv: int) -> int:
        return (sum(a.shape[0] for a in self._ctrl) - 3 * len(self._ctrl)) * int(subdiv)


def flatten_splines_numpy(ctrl: np.ndarray, stroke_off: np.ndarray, subdiv: int, alpha: float = 0.5, dtype=np.float64) -> np.ndarray:
    """``nb_spline_flatten_f32`` restated in numpy: [n, 5] rows (x0, y0, x1, y1, r) in ``dtype``.  Per span the knots are
    t0 = 0, t1 = |P1 - P0|^alpha, t2 = t1 + |P2 - P1|^alpha, t3 = t2 + |P3 - P2|^alpha; a sample is the pyramid A1..A3 -> B1, B2 -> C
    of linear interpolations over the knot intervals; sample k of a stroke closes segment k - 1 and opens segment k."""
    ctrl, subdiv = np.asarray(ctrl), int(subdiv)
    out = []
    for s in range(len(stroke_off) - 1):
        c = ctrl[int(stroke_off[s]):int(stroke_off[s + 1])].astype(dtype)
        p, rad = c[:, :2], c[:, 2]
        nsp = p.shape[0] - 3
        assert nsp >= 1, "every stroke needs at least 4 control points"
        k = np.arange(nsp * subdiv + 1)
        span = np.minimum(k // subdiv, nsp - 1)
        j = k - span * subdiv
        dx, dy = p[1:, 0] - p[:-1, 0], p[1:, 1] - p[:-1, 1]
        gap = np.power(np.sqrt(dx * dx + dy * dy), dtype(alpha)).astype(dtype)
        t0 = np.zeros(len(k), dtype)
        t1 = gap[span]
        t2 = t1 + gap[span + 1]
        t3 = t2 + gap[span + 2]
        t = np.where(j == subdiv, t2, t1 + (t2 - t1) * (j.astype(dtype) / dtype(subdiv)))

        def lerp(ta, tb, pa, pb):
            return ((tb - t) / (tb - ta))[:, None] * pa + ((t - ta) / (tb - ta))[:, None] * pb
        with np.errstate(divide="ignore", invalid="ignore"):
            a1, a2, a3 = lerp(t0, t1, p[span], p[span + 1]), lerp(t1, t2, p[span + 1], p[span + 2]), lerp(t2, t3, p[span + 2], p[span + 3])
            b1, b2 = lerp(t0, t2, a1, a2), lerp(t1, t3, a2, a3)
            pts = lerp(t1, t2, b1, b2)
        ks, kj = span[:-1], j[:-1]
        r = rad[ks + 1] + (rad[ks + 2] - rad[ks + 1]) * ((kj.astype(dtype) + dtype(0.5)) / dtype(subdiv))
        out.append(np.concatenate([pts[:-1], pts[1:], r[:, None]], axis=1).astype(dtype))
    return np.concatenate(out) if out else np.zeros((0, 5), dtype)


def raster_segments_numpy(segs: np.ndarray, out_shape: Tuple[int, int], offset=(0, 0), out: Optional[np.ndarray] = None) -> np.ndarray:
    """``nb_raster_segments_u8`` in float64: pixel (Y, X) is stroke (0) iff the distance from (X - off_x, Y - off_y) to the closed
    segment is <= r for some row; rows with a non-finite value or r < 0 draw nothing.  ``out`` given: darkened in place."""
    h, w = out_shape
    if out is None:
        out = np.full((h, w), 255, np.uint8)
    ys, xs = np.arange(h, dtype=np.float64) - offset[0], np.arange(w, dtype=np.float64) - offset[1]
    for x0, y0, x1, y1, r in np.asarray(segs, np.float64)[:, :5]:
        if not np.isfinite([x0, y0, x1, y1, r]).all() or r < 0:
            continue
        # the pixels of the segment's bounding box grown by r (and one more: the box is only a shortcut)
        ia, ib = np.searchsorted(ys, min(y0, y1) - r - 1), np.searchsorted(ys, max(y0, y1) + r + 1, side="right")
        ja, jb = np.searchsorted(xs, min(x0, x1) - r - 1), np.searchsorted(xs, max(x0, x1) + r + 1, side="right")
        if ib <= ia or jb <= ja:
            continue
        dx, dy = xs[None, ja:jb] - x0, ys[ia:ib, None] - y0
        ex, ey = x1 - x0, y1 - y0
        ee = ex * ex + ey * ey
        t = np.clip((dx * ex + dy * ey) / ee, 0.0, 1.0) if ee > 0 else 0.0
        fx, fy = dx - t * ex, dy - t * ey
        out[ia:ib, ja:jb][np.sqrt(fx * fx + fy * fy) - r <= 0] = 0
    return out


def raster_strokes_numpy(strokes: StrokeList, out_shape: Tuple[int, int], offset=(0, 0), subdiv: int = 8,
                         out: Optional[np.ndarray] = None) -> np.ndarray:
    """``TileOps.raster_strokes`` restated in numpy (float64 on the float32 stroke values): [h, w] uint8, 255 = background,
    0 = stroke, drawing position (0, 0) at pixel ``offset`` = (off_y, off_x); ``out`` given: darkened in place.  The route of an
    ``ops`` without the kernels (``TileOpsBase.raster_strokes``)."""
    ctrl, off = strokes.spline_control()
    segs = np.concatenate([strokes.polyline_segments()[:, :5].astype(np.float64), flatten_splines_numpy(ctrl, off, subdiv)])
    return raster_segments_numpy(segs, out.shape if out is not None else out_shape, offset, out)


def strokes_bounds(strokes: StrokeList, subdiv: int = 8) -> Optional[Tuple[int, int, int, int]]:
    """(y0, x0, y1, x1), end-exclusive, in drawing pixels: a box around every pixel the strokes can cover, from their points and
    radii on the host -- the polylines' segment rows and the splines' (a Catmull-Rom curve leaves the hull of its control points, so
    they are flattened here in float64), grown by the radius and one pixel for the device's fp32 flattening.  None: nothing to draw."""
    ctrl, off = strokes.spline_control()
    rows = np.concatenate([strokes.polyline_segments()[:, :5].astype(np.float64), flatten_splines_numpy(ctrl, off, subdiv)])
    rows = rows[np.isfinite(rows).all(axis=1) & (rows[:, 4] >= 0)]
    if rows.shape[0] == 0:
        return None
    grow = rows[:, 4] + 1
    x0, x1 = (np.minimum(rows[:, 0], rows[:, 2]) - grow).min(), (np.maximum(rows[:, 0], rows[:, 2]) + grow).max()
    y0, y1 = (np.minimum(rows[:, 1], rows[:, 3]) - grow).min(), (np.maximum(rows[:, 1], rows[:, 3]) + grow).max()
    lim = float(1 << 30)
    y0, x0, y1, x1 = (int(np.floor(np.clip(v, -lim, lim))) for v in (y0, x0, y1, x1))
    return y0, x0, y1 + 1, x1 + 1
