"""Painting-engine driver on the MI355X generator (SURVEY 8 rows e / f2; BASELINE configs 1 and 3).

Counterpart of the reference's ``PaintingHelper.render_stroke`` + ``FeatureCanvas`` (``forger/ui/brush.py:33-92,
95-398``), ``TriadGanPaintEngine._render_stroke_torch`` (``brush.py:731-805``), ``generate_stitching_crops``
(``forger/viz/style_transfer.py:15-48``) and the tile loop of ``forger/viz/paint_image_main.py:30-63, 145-192``.

The reference paints a canvas tile by tile: with feature blending every tile reads what earlier tiles left on the
``FeatureCanvas``.  That dependency is pointwise at the blending resolution, so this build runs ALL tiles through a
three-phase schedule with identical results (verified against the reference-generated canvases):

  phase 1  blocks b4..b(R/2) of every tile, batched           (``Generator`` split entry ``_stop_after``)
  phase 2  one launch replays the canvas blend tile after tile (``nb_canvas_replay_f32``)
  phase 3  last block + triad ToRGB + compositing, batched     (``_resume``), then one paste launch

Multi-GPU: the tile list is cut into contiguous per-rank ranges (``sharding.shard_bounds``); all three phases run on
the rank's own tiles only.  The blend of a tile reads what EARLIER tiles left under it, so a rank needs from the ranks
before it just the strips of their tiles that overlap its own (``sharding.halo_plan``: 20 px wide at R/2 for crop
margin 10, ~0.65 MB per neighbour pair at R=256) -- ONE ``all_to_all_single`` of those strips over RCCL/xGMI, started
as soon as the rank's boundary tiles are through phase 1 (they are scheduled first) and overlapped with the rest of
phase 1.  Each rank then replays its own tiles plus the received strips (``nb_canvas_replay_pieces_f32``) on the cells
its tiles cover, and the RGBA tiles are gathered on rank 0 for the paste.

Device work goes through ``TileOps`` (HIP kernels + the PyTorch-ROCm encoder).  There is no CPU fallback here: the
tests inject an oracle-backed ``TileOps`` stand-in to check the host logic and the sharded schedule on CPU.
"""
from __future__ import annotations

import contextlib
import dataclasses
import os
import time
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.distributed as dist

from . import _lib
from .sharding import HaloExchange, shard_bounds, shard_sizes

CELL_H, CELL_W = 4, 64          # NB_CELL_H / NB_CELL_W of include/neube_hip.h
PAINT_SLOT0 = 8                 # first generator workspace slot of the tiled schedule (TileOps._GRAPH_SLOT = 16 onwards: graphs)


# ------------------------------------------------------------------------------------------------
# host-side geometry / tiling helpers (numpy; no device work)
# ------------------------------------------------------------------------------------------------
def threshold_otsu(image: np.ndarray) -> float:
    """Otsu threshold of an integer image over its occupied value range -- the algorithm of
    ``skimage.filters.threshold_otsu`` (scikit-image 0.19, one bin per integer value), which
    ``forger/util/img_proc.py:66-71`` calls.  scikit-image is not installed in the build image, so this helper is
    NOT pinned against it (DESIGN.md says so).  ``nb_geom_prepare_u8`` computes the same threshold on the device."""
    img = np.asarray(image)
    if img.size == 0:
        raise ValueError("empty image")
    lo, hi = int(img.min()), int(img.max())
    if lo == hi:
        return float(lo)
    counts = np.bincount(img.ravel().astype(np.int64) - lo, minlength=hi - lo + 1).astype(np.float64)
    centers = np.arange(lo, hi + 1, dtype=np.float64)
    w1 = np.cumsum(counts)
    w2 = np.cumsum(counts[::-1])[::-1]
    m1 = np.cumsum(counts * centers) / np.maximum(w1, 1e-300)
    m2 = (np.cumsum((counts * centers)[::-1]) / np.maximum(w2[::-1], 1e-300))[::-1]
    var12 = w1[:-1] * w2[1:] * (m1[:-1] - m2[1:]) ** 2
    return float(centers[int(np.argmax(var12))])


def prepare_geometry_image(img: np.ndarray) -> np.ndarray:
    """``_read_any_geo`` (paint_image_main.py:30-55) from a decoded image array: gray / RGB / RGBA ->
    [H,W,1] uint8 with 255 = background, 0 = stroke (Otsu-thresholded)."""
    a = np.asarray(img).astype(np.float32)
    if a.ndim == 2:
        a = a[..., None]
    if a.shape[2] == 3:
        a = a[..., :3].mean(axis=2, dtype=np.float32)[..., None]
    elif a.shape[2] == 4:
        mean = a[..., :3].mean(axis=2, dtype=np.float32)
        alpha = a[..., 3] / np.float32(255)
        a = (mean * alpha + np.float32(255) * (1 - alpha))[..., None]
    mn = a.min()
    if mn > 0:
        a = a - mn
    mx = a.max()
    if 0 < mx < 255:
        a = a * np.float32(255.0 / float(mx))
    a8 = a.astype(np.uint8)
    return ((a8 > threshold_otsu(a8)).astype(np.float32) * 255).astype(np.uint8)


def read_geometry_image(fname: str) -> np.ndarray:
    from PIL import Image
    return prepare_geometry_image(np.array(Image.open(fname)))


def pad_geo(geo: np.ndarray, crop_margin: int) -> np.ndarray:
    """paint_image_main.py:58-61."""
    out = np.full((geo.shape[0] + crop_margin, geo.shape[1] + crop_margin, geo.shape[2]), 255, np.uint8)
    out[crop_margin:, crop_margin:, :] = geo
    return out


def generate_stitching_crops(stroke_image: np.ndarray, patch_width: int, mode: str = "all", overlap_margin: int = 15):
    """style_transfer.py:15-48: (y, x, P, P) crops at stride P - 2*overlap over the image padded with 255."""
    rwidth = patch_width - overlap_margin * 2
    assert rwidth > 0, "overlap margin too large for the patch width"
    h, w, ch = stroke_image.shape
    assert ch in (1, 2, 3, 4), f"Wrong shape {stroke_image.shape}"
    nrows, ncols = h // rwidth + 1, w // rwidth + 1
    padded = np.full((nrows * rwidth + patch_width, ncols * rwidth + patch_width, ch), 255, np.uint8)
    padded[:h, :w] = stroke_image
    crops = []
    for r in range(nrows):
        for c in range(ncols):
            y, x = r * rwidth, c * rwidth
            if mode == "all" or np.sum(padded[y:y + patch_width, x:x + patch_width] < 0.001) > 10:
                crops.append((y, x, patch_width, patch_width))
    return crops, padded


def stitching_grid(h: int, w: int, patch_width: int, overlap_margin: int) -> Tuple[int, int, int, int, int]:
    """(nrows, ncols, stride, padded_h, padded_w) of ``generate_stitching_crops`` for an [h, w] image (``nb_stitching_grid``)."""
    import ctypes as C
    v = [C.c_int() for _ in range(5)]
    _lib.check(_lib.lib().nb_stitching_grid(int(h), int(w), int(patch_width), int(overlap_margin), *[C.byref(x) for x in v]),
               "stitching_grid")
    return tuple(x.value for x in v)


def dirty_area_alpha(width: int, margin: int, crop_margin: int = 0) -> np.ndarray:
    """``PaintingHelper.generate_dirty_area_alpha`` (brush.py:159-187) for a dirty area spanning the whole tile:
    1 inside the rectangle inset by margin + crop_margin, linear fall-off of width ``margin`` outside (distance to the
    nearest edge; to the nearest corner in the corner regions), fp32 like the reference."""
    f32 = np.float32
    r0 = margin + crop_margin
    r1 = r0 + width - 2 * margin - 2 * crop_margin
    assert 0 <= r0 < r1 <= width, "blend margin + crop margin leave no interior"
    x = np.arange(width, dtype=f32)
    gy, gx = np.meshgrid(x, x, indexing="ij")
    dx = np.minimum((gx - f32(r0)) ** 2, (gx - f32(r1) + f32(1)) ** 2).astype(f32)
    dy = np.minimum((gy - f32(r0)) ** 2, (gy - f32(r1) + f32(1)) ** 2).astype(f32)
    d = (dx + dy).astype(f32)
    d[0:r0, r0:r1] = dy[0:r0, r0:r1]
    d[r1:, r0:r1] = dy[r1:, r0:r1]
    d[r0:r1, 0:r0] = dx[r0:r1, 0:r0]
    d[r0:r1, r1:] = dx[r0:r1, r1:]
    res = (f32(1) - np.sqrt(d).astype(f32) / f32(margin)).astype(f32)
    res[res < 0] = 0
    res[r0:r1, r0:r1] = 1
    return res


def build_cells(rects: np.ndarray, h: int, w: int) -> Tuple[np.ndarray, np.ndarray]:
    """CSR list of the rectangles (y0, x0, y1, x1; end-exclusive) touching each CELL_H x CELL_W cell of an h x w
    grid, in ascending rectangle order (include/neube_hip.h, "Cells").  Vectorised: canvases have thousands of tiles."""
    ncx, ncy = -(-w // CELL_W), -(-h // CELL_H)
    r = np.asarray(rects, np.int64).reshape(-1, 4)
    y0, x0 = np.maximum(r[:, 0], 0), np.maximum(r[:, 1], 0)
    y1, x1 = np.minimum(r[:, 2], h), np.minimum(r[:, 3], w)
    ok = (y1 > y0) & (x1 > x0)
    off = np.zeros(ncx * ncy + 1, np.int32)
    if not ok.any():
        return off, np.zeros(1, np.int32)
    t_idx = np.nonzero(ok)[0]
    cy0, cx0 = y0[ok] // CELL_H, x0[ok] // CELL_W
    ny, nx = (y1[ok] - 1) // CELL_H - cy0 + 1, (x1[ok] - 1) // CELL_W - cx0 + 1
    cnt = ny * nx
    rep = np.repeat(np.arange(len(t_idx)), cnt)                       # which rectangle each (cell, tile) pair belongs to
    local = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    cells = (cy0[rep] + local // nx[rep]) * ncx + cx0[rep] + local % nx[rep]
    tiles = t_idx[rep]
    order = np.lexsort((tiles, cells))                                # by cell, then ascending tile index
    np.cumsum(np.bincount(cells, minlength=ncx * ncy), out=off[1:])
    return off, tiles[order].astype(np.int32)


# ------------------------------------------------------------------------------------------------
# vector strokes (csrc/nb_strokes.hip): polylines and centripetal Catmull-Rom splines as capsule segments
# ------------------------------------------------------------------------------------------------
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
        import json
        return json.dumps(self.items)

    @classmethod
    def from_json(cls, text) -> "StrokeList":
        """From a JSON string or the list it decodes to."""
        import json
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


def raster_strokes_numpy(strokes: StrokeList, out_shape: Tuple[int, int], offset=(0, 0), subdiv: int = 8) -> np.ndarray:
    """``TileOps.raster_strokes`` restated in numpy (float64 on the float32 stroke values): [h, w] uint8, 255 = background,
    0 = stroke, drawing position (0, 0) at pixel ``offset`` = (off_y, off_x).  The route of an ``ops`` without the kernels."""
    ctrl, off = strokes.spline_control()
    segs = np.concatenate([strokes.polyline_segments()[:, :5].astype(np.float64), flatten_splines_numpy(ctrl, off, subdiv)])
    return raster_segments_numpy(segs, out_shape, offset)


# ------------------------------------------------------------------------------------------------
# compositing (csrc/nb_compose.hip): the two contracts of include/neube_hip.h restated in int64
# ------------------------------------------------------------------------------------------------
COMPOSE_MODES = {"paint": 0, "erase": 1}


def cell_box(box, h: int, w: int) -> Optional[Tuple[int, int, int, int]]:
    """(cell_x0, cell_y0, cells_x, cells_y): the cells of an h x w canvas that the pixel box (y0, x0, y1, x1; end-exclusive) touches,
    the whole canvas for None; None if the box misses the canvas."""
    if box is None:
        box = (0, 0, h, w)
    y0, x0 = max(0, int(box[0])) // CELL_H, max(0, int(box[1])) // CELL_W
    y1, x1 = -(-min(h, int(box[2])) // CELL_H), -(-min(w, int(box[3])) // CELL_W)
    if y1 <= y0 or x1 <= x0:
        return None
    return x0, y0, x1 - x0, y1 - y0


def over_tiles_numpy(canvas: np.ndarray, tiles: np.ndarray, dst_yx, crop: int, mode: int = 0, opacity: int = 255,
                     cells: Optional[Tuple[int, int, int, int]] = None) -> np.ndarray:
    """``nb_over_tiles_u8`` in int64, in place on ``canvas`` [h,w,4] uint8 (returned): per pixel the LAST of ``tiles`` [t,r,r,4]
    whose interior ``[crop, r-crop)^2`` at ``dst_yx[i] + crop`` covers it goes over (mode 0) or out of (mode 1) the pixel; only
    inside ``cells`` = (cell_x0, cell_y0, cells_x, cells_y), the whole canvas for None."""
    if mode not in (0, 1) or not 0 <= int(opacity) <= 255:
        raise ValueError(f"over_tiles: bad mode {mode} or opacity {opacity}")
    h, w = canvas.shape[:2]
    tiles = np.asarray(tiles)
    r, m = tiles.shape[1], int(crop)
    src = np.zeros((h, w, 4), np.uint8)
    cov = np.zeros((h, w), bool)
    for i, (y, x) in enumerate(np.asarray(dst_yx).reshape(-1, 2).tolist()):       # ascending: a later tile replaces an earlier one
        y0, x0, y1, x1 = max(0, y + m), max(0, x + m), min(h, y + r - m), min(w, x + r - m)
        if y1 > y0 and x1 > x0:
            src[y0:y1, x0:x1] = tiles[i, y0 - y:y1 - y, x0 - x:x1 - x]
            cov[y0:y1, x0:x1] = True
    if cells is not None:
        inside = np.zeros((h, w), bool)
        inside[cells[1] * CELL_H:(cells[1] + cells[3]) * CELL_H, cells[0] * CELL_W:(cells[0] + cells[2]) * CELL_W] = True
        cov &= inside
    s, d = src[cov].astype(np.int64), canvas[cov].astype(np.int64)
    ae = (s[:, 3] * int(opacity) + 127) // 255
    t = d[:, 3] * (255 - ae)
    out = d.copy()
    if mode == 1:
        out[:, 3] = (t + 127) // 255
    else:
        den = ae * 255 + t
        out[:, 3] = (den + 127) // 255
        num = s[:, :3] * (ae * 255)[:, None] + d[:, :3] * t[:, None] + (den // 2)[:, None]
        out[:, :3] = np.where(den[:, None] > 0, num // np.maximum(den, 1)[:, None], 0)
    canvas[cov] = out.astype(np.uint8)
    return canvas


def canvas_view_numpy(canvas: np.ndarray, y0: int, x0: int, h: int, w: int, k: int = 1, on_white: bool = False) -> np.ndarray:
    """``nb_canvas_view_u8`` in int64: the window of ``canvas`` [ch,cw,4] uint8 reduced by ``k`` -> [ceil(h/k), ceil(w/k), 4 | 3]."""
    ch, cw = canvas.shape[:2]
    if not (1 <= int(k) <= 16 and h >= 1 and w >= 1 and y0 >= 0 and x0 >= 0 and y0 + h <= ch and x0 + w <= cw):
        raise ValueError(f"canvas_view: bad factor {k} or window {h} x {w} at ({y0}, {x0}) of a {ch} x {cw} canvas")
    win = canvas[y0:y0 + h, x0:x0 + w].astype(np.int64)
    ys, xs = np.arange(0, h, k), np.arange(0, w, k)

    def blocks(a):
        return np.add.reduceat(np.add.reduceat(a, ys, axis=0), xs, axis=1)
    sa = blocks(win[..., 3])
    sc = blocks(win[..., :3] * win[..., 3:])
    n = np.outer(np.minimum(k, h - ys), np.minimum(k, w - xs))
    if on_white:
        den = (255 * n)[..., None]
        return ((sc + 255 * (den - sa[..., None]) + den // 2) // den).astype(np.uint8)
    colour = np.where(sa[..., None] > 0, (sc + (sa // 2)[..., None]) // np.maximum(sa, 1)[..., None], 0)
    return np.concatenate([colour, ((sa + n // 2) // n)[..., None]], axis=2).astype(np.uint8)


# ------------------------------------------------------------------------------------------------
# brush options (the subset of GanBrushOptions, brush.py:410-527, that the tiled path reads)
# ------------------------------------------------------------------------------------------------
class GanBrushOptions:
    def __init__(self, primary_color=None, secondary_color=None):
        self.color0 = self.color1 = self.canvas_color = None
        self.style_z = self.style_ws = self.style_id = None
        self.position = None
        self.custom_args: Dict = {}
        self.enable_uvs_mapping = False
        if primary_color is not None:
            self.set_color(0, primary_color)
        if secondary_color is not None:
            self.set_color(1, secondary_color)

    def set_position(self, x, y):
        self.position = torch.tensor([[int(y), int(x)]], dtype=torch.int64)

    def set_color(self, color_idx: int, in_color):
        c = None
        if in_color is not None:
            c = torch.as_tensor(np.asarray(in_color))
            c = c.to(torch.float32) / 255 if c.dtype == torch.uint8 else c.to(torch.float32)
            c = c.reshape(-1, 3)
        if color_idx == 0:
            self.color0 = c
        elif color_idx == 1:
            self.color1 = c
        elif color_idx == 2:
            self.canvas_color = c
        else:
            raise RuntimeError(f"Wrong color idx {color_idx}")

    def set_style(self, style_z, style_id=None):
        self.style_z, self.style_id, self.style_ws = style_z, style_id, None

    def set_style_w(self, style_w, style_id=None, custom_args=None):
        self.style_ws, self.style_id, self.style_z = style_w, style_id, None
        self.custom_args = {} if custom_args is None else custom_args

    def user_colors(self) -> Optional[torch.Tensor]:
        """[1,3(rgb),3(k)] with NaN = keep the generator's color (``prepare_colors``, brush.py:514-527)."""
        if self.color0 is None and self.color1 is None and self.canvas_color is None:
            return None
        uc = torch.full([1, 3, 3], float("nan"), dtype=torch.float32)
        for k, c in enumerate((self.color0, self.color1, self.canvas_color)):
            if c is not None:
                uc[0, :, k] = c[0]
        return uc


# ------------------------------------------------------------------------------------------------
# device operations (HIP)
# ------------------------------------------------------------------------------------------------
def _p(t):
    return None if t is None else t.data_ptr()


class TileOpsBase:
    """The scheduling hooks ``PaintingHelper`` calls on its ``ops``, with defaults that do nothing: one stream, no workspaces to
    prepare, no noise sets, no captured graphs.  ``TileOps`` overrides all of them; the CPU stand-ins of the
    tests derive from this class and define the device operations (``geom_tiles``, ``encode``, ``head`` / ``tail`` / ``full``, the
    canvas operations) only."""
    n_streams = 1
    stream_policy = 0
    graph_single = None          # None: no graphs to switch on (render_stroke leaves it alone)

    def stream(self, k: int):
        return contextlib.nullcontext()

    def comm_stream(self):
        return contextlib.nullcontext()

    def join_streams(self, tensors=()) -> None:
        pass

    def join_comm(self, tensors=()) -> None:
        pass

    def prepare(self, n: int, slots) -> None:
        pass

    def choose_streams(self, n: int, render_mode: str = "clear") -> None:
        pass

    def brush_noise(self):
        """None: this ops has no noise sets, and is never handed one."""
        return None

    def to_host(self, t: torch.Tensor) -> np.ndarray:
        return t.cpu().numpy()

    # -- compositing: the numpy restatements, on host tensors (``TileOps`` runs the kernels of csrc/nb_compose.hip) --
    def over_tiles(self, canvas, tiles_u8, dst_yx, crop, cell_off, cell_tiles, box=None, mode: int = 0, opacity: int = 255) -> None:
        """``tiles_u8`` [t,r,r,4] over (mode 0) or out of (mode 1) ``canvas`` [h,w,4], in place, inside the cells that the pixel box
        (y0, x0, y1, x1) touches (None: everywhere).  The cell lists are those of ``paste``."""
        h, w = canvas.shape[:2]
        cells = cell_box(box, h, w)
        if cells is not None:
            over_tiles_numpy(canvas.numpy(), tiles_u8.numpy(), dst_yx.numpy(), crop, mode, opacity, cells)

    def canvas_view(self, canvas, y0: int, x0: int, h: int, w: int, k: int = 1, on_white: bool = False) -> torch.Tensor:
        """[ceil(h/k), ceil(w/k), 4 | 3] uint8: the window of the RGBA canvas at (y0, x0) reduced by ``k``."""
        return torch.from_numpy(canvas_view_numpy(canvas.numpy(), y0, x0, h, w, k, on_white))


class TileOps(TileOpsBase):
    """What the tiled schedule needs from the device: the HIP generator split in two, the geometry encoder, and the
    canvas kernels of ``csrc/nb_canvas.hip``."""
    _comm = None                 # the halo exchange's side stream (comm_stream creates it)
    _prep_ws = None              # workspace of nb_geom_prepare_u8 (prepare_geometry creates it)

    def __init__(self, G, encoder, device=None):
        self.G, self.encoder = G, encoder
        self.device = torch.device(device) if device is not None else G.synthesis.get_last_block().conv1.weight.device
        if self.device.type != "cuda":
            raise _lib.NeubeHipError("the painting engine needs the generator on a GPU (no CPU path in this build)")
        self.patch_width = G.img_resolution
        self.cfg = G.cfg
        # the encoder computes in the generator's arithmetic: fp8 correction operands between its layers only when the generator
        # itself runs "f8" (its features then carry ~3e-4 instead of ~2e-5 absolute error on O(5) values)
        if hasattr(encoder, "arith"):
            encoder.arith = "f8" if getattr(G.synthesis, "conv_mode", None) == "f8" else "h3"
        self._rr = {}                # stream count -> pipeline.RoundRobinStreams (created at first use, kept across probes)
        self._graphs, self._graph_epoch, self._capturing = {}, None, False

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    # -- inputs --
    def to_device(self, a: np.ndarray) -> torch.Tensor:
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.device, non_blocking=True)

    def to_host(self, t: torch.Tensor) -> np.ndarray:
        """Device tensor -> numpy through a pinned buffer (the caching host allocator recycles it once the array dies)."""
        host = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
        host.copy_(t, non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        return host.numpy()

    def geom_tiles(self, geom_dev: torch.Tensor, tile_yx: torch.Tensor) -> torch.Tensor:
        gh, gw = geom_dev.shape
        t, r = tile_yx.shape[0], self.patch_width
        out = torch.empty([t, 1, r, r], dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().nb_geom_tiles_f32(_p(geom_dev), gh, gw, _p(tile_yx), t, r, _p(out), self._stream()),
                       "geom_tiles")
        return out

    lazy_geometry = True       # hand the generator a geometry provider (encoder output straight into the layer operands)

    def encode(self, geom: torch.Tensor):
        if self.lazy_geometry and hasattr(self.encoder, "lazy"):
            return self.encoder.lazy(geom)
        return self.encoder.encode(geom)

    def prepare(self, n: int, slots) -> None:
        """Create the generator workspaces of ``slots`` for batches of ``n`` on the CALLER's stream, before the batch streams fork
        (a workspace is otherwise created by the first batch that needs it, on that batch's stream, while the other stream is
        already running)."""
        for sl in slots:
            self.G.synthesis._get_plan(n, self.device, sl)

    def map_style(self, z=None, ws=None) -> torch.Tensor:
        if ws is not None:
            return ws.to(self.device, torch.float32)
        return self.G.mapping(z.to(self.device), None)

    # -- generator halves --
    # ``slot``: which of the generator's per-batch workspaces to use -- consecutive batches alternate between two HIP
    # streams (``stream``/``join_streams``), each with its own workspace, so that one batch's kernel tails and small
    # launches are covered by the other batch's work
    # ``noise_set``: the brush's noise buffers (``networks.BrushNoise``, ``brush_noise()`` below; None = the checkpoint's noise).  Its
    # identity is part of a graph's key, its contents are not: the set's addresses are fixed, so a captured pass renders whatever the
    # set holds when it is replayed.
    def brush_noise(self):
        return self.G.synthesis.brush_noise()

    @staticmethod
    def _set_key(noise_set):
        return None if noise_set is None else id(noise_set)       # (the graph's closure keeps the set alive: the id stays its own)

    def head(self, ws, geom_feats, positions, stop_res: int, slot: int = 0, noise_set=None) -> torch.Tensor:
        if self._use_graph(ws):
            return self._graphed(("head", stop_res, self._set_key(noise_set)), [ws, geom_feats[0], geom_feats[1], positions],
                                 lambda w, g0, g1, ps: self.head(w, [g0, g1], ps, stop_res, slot=self._GRAPH_SLOT, noise_set=noise_set))
        return self.G.forward_pre_mapped(ws, geom_feats, positions=positions, noise_mode="const", _stop_after=stop_res,
                                         _plan_slot=slot, noise_set=noise_set)

    def tail(self, ws, feats, geom_feats, positions, resume_res: int, render_mode, user_colors, sfactor=None,
             slot: int = 0, noise_set=None) -> torch.Tensor:
        if self._use_graph(ws) and (sfactor is None or torch.is_tensor(sfactor)):
            return self._graphed(("tail", resume_res, render_mode, self._set_key(noise_set)),
                                 [ws, feats, geom_feats[0], geom_feats[1], positions, user_colors, sfactor],
                                 lambda w, f, g0, g1, ps, uc, sf: self.tail(w, f, [g0, g1], ps, resume_res, render_mode, uc, sf,
                                                                           slot=self._GRAPH_SLOT + 1, noise_set=noise_set))
        u8, _, _ = self.G.render_triad(ws=ws, geom_feature=geom_feats, positions=positions, render_mode=render_mode,
                                       user_colors=user_colors, sfactor=sfactor, _resume=(resume_res, feats), _plan_slot=slot,
                                       noise_set=noise_set)
        return u8

    def full(self, ws, geom_feats, positions, render_mode, user_colors, sfactor=None, slot: int = 0, noise_set=None) -> torch.Tensor:
        if self._use_graph(ws) and (sfactor is None or torch.is_tensor(sfactor)):
            return self._graphed(("full", render_mode, self._set_key(noise_set)),
                                 [ws, geom_feats[0], geom_feats[1], positions, user_colors, sfactor],
                                 lambda w, g0, g1, ps, uc, sf: self.full(w, [g0, g1], ps, render_mode, uc, sf,
                                                                         slot=self._GRAPH_SLOT + 2, noise_set=noise_set))
        u8, _, _ = self.G.render_triad(ws=ws, geom_feature=geom_feats, positions=positions, render_mode=render_mode,
                                       user_colors=user_colors, sfactor=sfactor, _plan_slot=slot, noise_set=noise_set)
        return u8

    # -- hipGraph replay of the generator passes of ONE tile (interactive strokes) --
    # An interactive stroke is bound by the ~0.2 ms of Python each eager generator pass costs, not by the device.  With
    # ``graph_single`` set (PaintingHelper.render_stroke does), the passes of a single tile are captured once per call
    # signature into hipGraphs that own a workspace slot; a call then copies its inputs into the graph's static
    # tensors and replays.  The returned tensor is the graph's output buffer: valid until the next call of that pass.
    graph_single = False
    _GRAPH_SLOT = 16

    def _use_graph(self, ws) -> bool:
        return (self.graph_single and not self._capturing and ws.shape[0] == 1 and len(self.cfg.geom_feature_channels) == 2
                and not torch.cuda.is_current_stream_capturing())

    def _graphed(self, key, tensors, fn):
        packed = self.G.synthesis.packed
        if self._graph_epoch is not packed:                   # weights were (re)loaded / moved: captured pointers are stale
            self._graphs, self._graph_epoch = {}, packed
        key = key + tuple(None if t is None else (tuple(t.shape), t.dtype) for t in tensors)
        ent = self._graphs.get(key)
        if ent is None:
            statics = [None if t is None else t.detach().clone() for t in tensors]
            self._capturing = True
            try:
                cur = torch.cuda.current_stream(self.device)
                side = torch.cuda.Stream(device=self.device)
                side.wait_stream(cur)
                with torch.cuda.stream(side):                # creates the slot's workspace, packs weights, warms the kernels
                    for _ in range(2):
                        fn(*statics)
                cur.wait_stream(side)
                torch.cuda.synchronize(self.device)
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    out = fn(*statics)
            finally:
                self._capturing = False
            ent = (graph, statics, out)
            self._graphs[key] = ent
        graph, statics, out = ent
        for s_, t in zip(statics, tensors):
            if s_ is not None:
                s_.copy_(t, non_blocking=True)
        graph.replay()
        return out

    n_streams = 2
    # 0 = choose n_streams by a probe the first time a multi-batch canvas is painted (choose_streams); 1 / 2 / 3 = fixed.
    # Alternating batches over HIP streams lets one batch's kernel tails and small launches run under the other's big ones, which
    # is worth +5..10 % on most boxes -- and cost 14 % on the box of the round-3 driver run (three chains of 156 KB-LDS workgroups
    # evicting each other at kernel boundaries), so the schedule measures instead of assuming.
    stream_policy = int(os.environ.get("NB_CANVAS_STREAMS", "0"))
    stream_probe = None          # what choose_streams measured: {"ms_per_batch": {1: .., 2: ..}, "chosen": n, "batch": n}

    def _set_n_streams(self, k: int) -> None:
        """Change the number of batch streams (every count keeps its own ``RoundRobinStreams``; ``stream(k)`` indexes the current one)."""
        self.n_streams = k

    def _round_robin(self):
        """The scheduler of the generator's throughput mode (``pipeline.RoundRobinStreams``, also behind ``ConcurrentTriadSteps`` /
        ``bench.py``): batch b runs on stream b % n_streams with workspace slot PAINT_SLOT0 + b % n_streams."""
        from .pipeline import RoundRobinStreams
        rr = self._rr.get(self.n_streams)
        if rr is None:
            rr = self._rr[self.n_streams] = RoundRobinStreams(self.device, self.n_streams, PAINT_SLOT0)
        return rr

    def choose_streams(self, n: int, render_mode: str = "clear") -> int:
        """Pick the number of batch streams for batches of ``n`` tiles: the fixed policy, or -- once per TileOps and batch size --
        two streams unless a probe -- three interleaved rounds of six synthetic batches on 1 and on 2 streams, best of three each, full
        generator passes with random styles and geometry features, ~80 ms -- shows them more than 3 % slower.  Sets ``n_streams``; the probe's figures stay in ``stream_probe`` (tools/bench_canvas.py reports them)."""
        if self.stream_policy > 0:
            self._set_n_streams(self.stream_policy)
            return self.n_streams
        if self.stream_probe is not None and self.stream_probe.get("batch") == n:
            return self.n_streams
        cfg, dev = self.cfg, self.device
        gen = torch.Generator(device="cpu").manual_seed(1234)
        ws = torch.randn([n, cfg.num_ws, cfg.w_dim], generator=gen).to(dev)
        geom = [torch.randn([n, c, r, r], generator=gen).to(dev) for c, r in zip(cfg.geom_feature_channels, cfg.geom_feature_resolutions)]
        pos = torch.zeros([n, 2], dtype=torch.int64, device=dev)
        times = {1: [], 2: []}

        def run(k, batches):
            # (each stream count keeps its own side streams across the interleaved rounds)
            self._set_n_streams(k)
            self.prepare(n, sorted({PAINT_SLOT0 + i % k for i in range(k)}))
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            outs = []
            for b in range(batches):
                with self.stream(b):
                    outs.append(self.full(ws, geom, pos, render_mode, None, None, slot=PAINT_SLOT0 + b % k))
            self.join_streams(outs)
            torch.cuda.synchronize(dev)
            return (time.perf_counter() - t0) / batches * 1e3
        run(1, 2); run(2, 4)                             # workspaces, code objects, clocks
        for _ in range(3):                               # interleaved, best of three each: a single pair of short runs was off by
            times[1].append(run(1, 6))                   # +-7 % between processes on one box (r04 collection: 1.89 vs 2.02 ms, then
            times[2].append(run(2, 6))                   # 1.87 vs 1.77 ms a minute later), more than the effect it is meant to see
        times = {k: min(v) for k, v in times.items()}
        # two streams unless they are clearly slower HERE.  The probe renders generator passes only; in the canvas job, where encoder,
        # canvas kernels and copies sit between them, the second stream is worth 5-7 % on every box measured (same-box A/Bs of the
        # 4096^2 job in round 4: 44.4 -> 42.2, 44.1 -> 41.0, 43.8 -> 40.8 ms) while their probes said 1.81 -> 1.79, 2.08 -> 1.81 and
        # 1.85 -> 1.87 ms per batch: a probe within noise must not cost the job its overlap; a box that loses with concurrent chains
        # (the round-3 driver run saw three streams 14 % below one) shows it as > 3 % here
        best = 1 if times[2] > 1.03 * times[1] else 2
        self._set_n_streams(best)
        self.stream_probe = {"ms_per_batch": {str(k): round(v, 4) for k, v in times.items()}, "chosen": best, "batch": n}
        return best

    def stream(self, k: int):
        """Context manager: work of batch k goes to side stream k % n_streams (which first waits for the caller's)."""
        return self._round_robin().stream(k)

    def join_streams(self, tensors=()):
        """The caller's stream waits for the side streams; ``tensors`` produced there are about to be read here."""
        rr = self._rr.get(self.n_streams)
        if rr is not None:
            rr.join(tensors)
        else:
            main = torch.cuda.current_stream(self.device)
            for t in tensors:
                if torch.is_tensor(t) and t.is_cuda:
                    t.record_stream(main)

    def comm_stream(self):
        """Context manager for the halo exchange: a side stream that first waits for everything enqueued so far on the
        batch streams (the boundary tiles' phase 1), so that packing + the collective overlap the remaining batches."""
        if self._comm is None:
            self._comm = torch.cuda.Stream(device=self.device)
        self._comm.wait_stream(torch.cuda.current_stream(self.device))
        rr = self._rr.get(self.n_streams)
        for st in (rr.streams if rr is not None else []):
            self._comm.wait_stream(st)
        return torch.cuda.stream(self._comm)

    def join_comm(self, tensors=()):
        if self._comm is not None:
            main = torch.cuda.current_stream(self.device)
            main.wait_stream(self._comm)
            for t in tensors:
                if torch.is_tensor(t) and t.is_cuda:
                    t.record_stream(main)

    def background_weight(self, ws, geom_feats) -> torch.Tensor:
        """S = uvs[:, 2:3] of an un-positioned render (what StyleUVSMapper calibrates on, mapper.py:74-87)."""
        _, dbg = self.G.forward_pre_mapped(ws, geom_feats, return_debug_data=True, noise_mode="const")
        return dbg["uvs"][:, 2:3]

    # -- canvas kernels --
    def new_feature_canvas(self, c, hc, wc):
        return (torch.zeros([1, c, hc, wc], dtype=torch.float32, device=self.device),
                torch.zeros([hc, wc], dtype=torch.uint8, device=self.device))

    def replay(self, tiles, tile_yx, alpha0, crop, canvas, mask, cell_off, cell_tiles, box=None) -> torch.Tensor:
        """In place on ``tiles`` and ``canvas``; returns the new mask buffer.  ``box`` = (y0, x0, y1, x1) canvas pixels
        that contain every tile (an interactive stroke replays one tile on a large canvas): only those cells run."""
        t, c, hw, _ = tiles.shape
        hc, wc = mask.shape
        with torch.cuda.device(self.device):
            if box is not None:
                y0, x0 = max(0, box[0]) // CELL_H, max(0, box[1]) // CELL_W
                y1, x1 = -(-min(hc, box[2]) // CELL_H), -(-min(wc, box[3]) // CELL_W)
                if y1 <= y0 or x1 <= x0:
                    return mask
                mask_out = mask.clone()
                _lib.check(_lib.lib().nb_canvas_replay_box_f32(_p(tiles), t, c, hw, _p(tile_yx), _p(alpha0), crop, _p(canvas),
                                                               _p(mask), _p(mask_out), hc, wc, _p(cell_off), _p(cell_tiles),
                                                               x0, y0, x1 - x0, y1 - y0, self._stream()), "canvas_replay")
                return mask_out
            mask_out = torch.empty_like(mask)
            _lib.check(_lib.lib().nb_canvas_replay_f32(_p(tiles), t, c, hw, _p(tile_yx), _p(alpha0), crop, _p(canvas),
                                                       _p(mask), _p(mask_out), hc, wc, _p(cell_off), _p(cell_tiles),
                                                       self._stream()), "canvas_replay")
        return mask_out

    def replay_pieces(self, pieces, hw, alpha0, crop, canvas, mask, cell_off, cell_pieces, box) -> torch.Tensor:
        """The replay over tile pieces (multi-GPU halo exchange).  ``pieces`` = [(view [C,h,w] with unit column stride,
        cy, cx, ly0, lx0), ...] in paint order; in place on the views and ``canvas``; returns the new mask buffer.
        ``box`` = (y0, x0, y1, x1) canvas pixels containing every piece."""
        import ctypes as C
        hc, wc = mask.shape
        c = pieces[0][0].shape[0]
        arr = (_lib.NbTilePiece * len(pieces))()
        for i, (v, cy, cx, ly0, lx0) in enumerate(pieces):
            assert v.dtype == torch.float32 and v.stride(2) == 1 and v.shape[0] == c
            arr[i] = _lib.NbTilePiece(v.data_ptr(), v.stride(0), v.stride(1), cy, cx, v.shape[1], v.shape[2], ly0, lx0)
        table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(self.device, non_blocking=True)
        y0, x0 = max(0, box[0]) // CELL_H, max(0, box[1]) // CELL_W
        y1, x1 = -(-min(hc, box[2]) // CELL_H), -(-min(wc, box[3]) // CELL_W)
        if y1 <= y0 or x1 <= x0:
            return mask
        mask_out = mask.clone()
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().nb_canvas_replay_pieces_f32(_p(table), len(pieces), c, hw, _p(alpha0), crop, _p(canvas),
                                                              _p(mask), _p(mask_out), hc, wc, _p(cell_off), _p(cell_pieces),
                                                              x0, y0, x1 - x0, y1 - y0, self._stream()), "canvas_replay_pieces")
        return mask_out

    def paste(self, canvas_u8, tiles_u8, dst_yx, crop, cell_off, cell_tiles) -> None:
        t, r = tiles_u8.shape[0], tiles_u8.shape[1]
        h, w = canvas_u8.shape[:2]
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().nb_paste_tiles_u8(_p(tiles_u8), t, r, _p(dst_yx), crop, _p(canvas_u8), h, w,
                                                    _p(cell_off), _p(cell_tiles), self._stream()), "paste_tiles")

    # -- drawing preparation (csrc/nb_geomprep.hip) --
    def prepare_geometry(self, img, out_shape=None, offset=(0, 0)) -> torch.Tensor:
        """``prepare_geometry_image(img)[..., 0]`` computed on the device and placed at ``offset`` of a [out_h, out_w] uint8
        buffer that is 255 elsewhere (``nb_geom_prepare_u8``).  ``img``: decoded drawing, uint8 [H,W], [H,W,3] or [H,W,4],
        numpy (uploaded here) or a device tensor."""
        if not torch.is_tensor(img):
            img = np.asarray(img)
            if img.dtype != np.uint8:
                raise ValueError(f"prepare_geometry: the drawing must be uint8, got {img.dtype}")
            img = self.to_device(img)
        if img.dtype != torch.uint8 or img.dim() not in (2, 3):
            raise ValueError(f"prepare_geometry: uint8 [H,W] or [H,W,C] expected, got {img.dtype} {tuple(img.shape)}")
        img = img.contiguous()
        h, w = img.shape[:2]
        ch = 1 if img.dim() == 2 else img.shape[2]
        out_h, out_w = (h, w) if out_shape is None else out_shape
        out = torch.empty([out_h, out_w], dtype=torch.uint8, device=self.device)
        if self._prep_ws is None:
            self._prep_ws = torch.empty([_lib.NB_GEOM_PREP_WS_BYTES // 4], dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().nb_geom_prepare_u8(_p(img), h, w, ch, _p(out), out_h, out_w, int(offset[0]), int(offset[1]),
                                                     _p(self._prep_ws), self._stream()), "geom_prepare")
        return out

    def stroke_counts(self, geom_dev: torch.Tensor, r: int, stride: int, nrows: int, ncols: int) -> torch.Tensor:
        """[nrows, ncols] int32 on the device: stroke pixels (== 0) in the r x r window of every tile (``nb_tile_stroke_counts_u8``)."""
        gh, gw = geom_dev.shape
        counts = torch.empty([nrows, ncols], dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().nb_tile_stroke_counts_u8(_p(geom_dev), gh, gw, r, stride, nrows, ncols, _p(counts), self._stream()),
                       "tile_stroke_counts")
        return counts

    def composite_on_white(self, canvas: torch.Tensor, y0: int, x0: int, h: int, w: int) -> torch.Tensor:
        """[h, w, 3] uint8: the window of the RGBA canvas at (y0, x0) over white (``nb_composite_on_white_u8``)."""
        ch, cw = canvas.shape[:2]
        out = torch.empty([h, w, 3], dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().nb_composite_on_white_u8(_p(canvas), ch, cw, y0, x0, h, w, _p(out), self._stream()),
                       "composite_on_white")
        return out

    # -- compositing (csrc/nb_compose.hip) --
    def over_tiles(self, canvas, tiles_u8, dst_yx, crop, cell_off, cell_tiles, box=None, mode: int = 0, opacity: int = 255) -> None:
        """``tiles_u8`` [t,r,r,4] over (mode 0) or out of (mode 1) ``canvas`` [h,w,4], in place, inside the cells that the pixel box
        (y0, x0, y1, x1) touches (None: everywhere).  The cell lists are those of ``paste`` (``nb_over_tiles_u8``)."""
        t, r = tiles_u8.shape[0], tiles_u8.shape[1]
        h, w = canvas.shape[:2]
        cells = cell_box(box, h, w)
        if cells is None:
            return
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().nb_over_tiles_u8(_p(tiles_u8), t, r, _p(dst_yx), crop, _p(canvas), h, w, _p(cell_off), _p(cell_tiles),
                                                   *cells, int(mode), int(opacity), self._stream()), "over_tiles")

    def canvas_view(self, canvas, y0: int, x0: int, h: int, w: int, k: int = 1, on_white: bool = False) -> torch.Tensor:
        """[ceil(h/k), ceil(w/k), 4 | 3] uint8: the window of the RGBA canvas at (y0, x0) reduced by ``k`` (``nb_canvas_view_u8``)."""
        ch, cw = canvas.shape[:2]
        k = int(k)
        if not 1 <= k <= 16:
            raise ValueError(f"canvas_view: factor {k} outside 1..16")
        out = torch.empty([-(-int(h) // k), -(-int(w) // k), 3 if on_white else 4], dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().nb_canvas_view_u8(_p(canvas), ch, cw, int(y0), int(x0), int(h), int(w), k, int(bool(on_white)), _p(out),
                                                    self._stream()), "canvas_view")
        return out

    # -- vector strokes (csrc/nb_strokes.hip) --
    spline_alpha = 0.5           # centripetal Catmull-Rom, the reference's default (curve.py:24)

    def stroke_segments(self, strokes: StrokeList, subdiv: int = 8) -> torch.Tensor:
        """[n, SEG_PITCH] float32 on the device: the polylines' segment rows (uploaded) followed by the splines' (control points
        uploaded, cut into ``subdiv`` pieces per span by ``nb_spline_flatten_f32``).  Kilobytes cross PCIe."""
        poly = strokes.polyline_segments()
        ctrl, off = strokes.spline_control()
        n_poly, n_spl = poly.shape[0], strokes.spline_segment_count(subdiv)
        segs = torch.empty([n_poly + n_spl, SEG_PITCH], dtype=torch.float32, device=self.device)
        if n_poly:
            segs[:n_poly].copy_(torch.from_numpy(poly), non_blocking=True)
        if n_spl:
            d_ctrl, d_off = self.to_device(ctrl), self.to_device(off)
            with torch.cuda.device(self.device):
                _lib.check(_lib.lib().nb_spline_flatten_f32(_p(d_ctrl), _p(d_off), ctrl.shape[0], len(off) - 1, int(subdiv),
                                                            float(self.spline_alpha), _p(segs[n_poly:]), n_spl, self._stream()),
                           "spline_flatten")
        return segs

    def raster_segments(self, segs: torch.Tensor, out_shape=None, offset=(0, 0), out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``nb_raster_segments_u8`` on device segment rows [n, SEG_PITCH]: a new [out_h, out_w] uint8 geometry (255 = background,
        0 = stroke), or, with ``out`` given, the strokes darkened onto that tensor and everything else left as it is."""
        if segs.dtype != torch.float32 or segs.dim() != 2 or segs.shape[1] != SEG_PITCH or not segs.is_contiguous():
            raise ValueError(f"raster_segments: contiguous float32 [n, {SEG_PITCH}] expected, got {segs.dtype} {tuple(segs.shape)}")
        clear = out is None
        if clear:
            out = torch.empty([int(out_shape[0]), int(out_shape[1])], dtype=torch.uint8, device=self.device)
        elif out.dtype != torch.uint8 or out.dim() != 2 or not out.is_contiguous() or out.device != segs.device:
            raise ValueError(f"raster_segments: out must be a contiguous uint8 [H,W] device tensor, got {out.dtype} {tuple(out.shape)}")
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().nb_raster_segments_u8(_p(segs) if segs.shape[0] else None, segs.shape[0], _p(out), out.shape[0],
                                                        out.shape[1], int(offset[0]), int(offset[1]), int(clear), self._stream()),
                       "raster_segments")
        return out

    def raster_strokes(self, strokes: StrokeList, out_shape=None, offset=(0, 0), out: Optional[torch.Tensor] = None,
                       subdiv: int = 8) -> torch.Tensor:
        """The strokes as [out_h, out_w] uint8 geometry on the device (255 = background, 0 = stroke), drawing position (0, 0) at
        pixel ``offset`` = (off_y, off_x): splines are flattened on the device, and polyline and spline segments are rasterised in
        one ``nb_raster_segments_u8`` launch.  ``out`` given: the strokes are added to that geometry (every other byte untouched)."""
        return self.raster_segments(self.stroke_segments(strokes, subdiv), out_shape, offset, out)


# ------------------------------------------------------------------------------------------------
# clear-background mapping (reference: StyleUVSMapper, forger/ui/mapper.py:16-72, 117-135)
# ------------------------------------------------------------------------------------------------
class StyleUVSMapper:
    """Per-style scale ``sfactor`` that stretches the background weight S of the triad so that clear background
    renders fully transparent; the remap itself (``_map_style_s``) is fused into the ToRGB launch
    (``nb_torgb_triad_f32(sfactor=...)``).  The reference calibrates on five bundled drawings at two stroke widths
    (``*_rad016.png`` / ``*_rad025.png``); they are data files of the reference, so the caller supplies them."""

    def __init__(self, ops, cal_medium: Optional[np.ndarray] = None, cal_thick: Optional[np.ndarray] = None):
        self.ops = ops
        self.sfactors: Dict = {}
        self.geom_feature = self.bmask = None
        if cal_medium is not None:
            self.set_calibration(cal_medium, cal_thick)

    def set_calibration(self, cal_medium: np.ndarray, cal_thick: np.ndarray):
        """[k,R,R] uint8 drawings, 0 = stroke: medium strokes are rendered, thick ones define "surely background"."""
        geo = (self.ops.to_device(np.asarray(cal_medium, np.uint8)).to(torch.float32) / 255).unsqueeze(1)
        self.geom_feature = self.ops.encode(geo)
        self.bmask = (self.ops.to_device(np.asarray(cal_thick, np.uint8)).to(torch.float32) / 255).unsqueeze(1) > 0.99
        self.sfactors = {}

    def get_sfactor(self, opts) -> torch.Tensor:
        if opts.style_id is not None and opts.style_id in self.sfactors:
            return self.sfactors[opts.style_id]
        if self.geom_feature is None:
            raise RuntimeError("StyleUVSMapper: no calibration drawings set (set_calibration)")
        n = self.geom_feature[0].shape[0]
        ws = self.ops.map_style(z=opts.style_z, ws=opts.style_ws).expand(n, -1, -1).contiguous()
        S = self.ops.background_weight(ws, self.geom_feature)
        val = torch.stack([torch.topk(S[i][self.bmask[i]], k=15)[0].min() for i in range(n)]).min()
        sfactor = 1 / val
        if opts.style_id is not None:
            self.sfactors[opts.style_id] = sfactor
        return sfactor


def _on_white_torch(ops, rgba: torch.Tensor) -> torch.Tensor:
    """paint_image_main.py:179-183 as a torch expression (3 channels out): what ``nb_composite_on_white_u8`` computes, for an
    ``ops`` without that kernel."""
    # alpha = a / 255 through a host-computed table: device division is not correctly rounded
    lut = ops.to_device(np.arange(256, dtype=np.float32) / np.float32(255))
    a = lut[rgba[..., 3:].to(torch.int64)]
    return (rgba[..., :3].to(torch.float32) * a + 255 * (1 - a)).clip(0, 255).to(torch.uint8)


# ------------------------------------------------------------------------------------------------
# the painting helper
# ------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class _Job:
    """What one ``PaintingHelper._schedule`` call decides up front and every phase reads."""
    rank: int
    world: int
    sharded: bool                      # the multi-rank schedule: halo exchange, pieces replay, tile gather
    T: int                             # tiles of the call; this rank owns t0..t1 (``bounds``: every rank's range)
    bounds: List[Tuple[int, int]]
    t0: int
    t1: int
    geom_dev: torch.Tensor             # the geometry image on the device
    ws1: torch.Tensor                  # the one brush style of all tiles
    user_dev: Optional[torch.Tensor]   # the user's colours on the device
    sfac: Optional[torch.Tensor]       # UVS factor
    nkw: dict                          # {"noise_set": ...} for a projected brush, else empty
    own_yx: Optional[torch.Tensor]     # geometry corners / noise positions of my tiles, on the device
    own_pos: Optional[torch.Tensor]
    batches: List[Tuple[int, int]]     # (b0, b1) ranges of my tiles; batch k runs under on_stream(k) with workspace plan_slot(k)
    on_stream: Callable
    join: Callable
    plan_slot: Callable

    @property
    def n_own(self) -> int:
        return self.t1 - self.t0

    def style(self, n: int) -> torch.Tensor:
        return self.ws1.expand(n, -1, -1).contiguous()

    def pos(self, b0: int, b1: int) -> Optional[torch.Tensor]:
        return None if self.own_pos is None else self.own_pos[b0:b1]

    def colors(self, n: int) -> Optional[torch.Tensor]:
        return None if self.user_dev is None else self.user_dev.expand(n, -1, -1).contiguous()


class PaintingHelper:
    """Server-side canvas state + rendering (reference: ``PaintingHelper``, brush.py:95-398).

    ``render_stroke`` keeps the reference's one-tile-per-call contract (interactive strokes); ``render_tiles`` takes a
    whole tile list through the three-phase schedule and is what ``paint_image`` uses."""

    feature_blending_margin = 16

    def __init__(self, ops: TileOps, batch: int = 32, group=None, uvs_mapper: Optional[StyleUVSMapper] = None):
        self.ops = ops
        self.uvs_mapper = uvs_mapper
        self.batch = int(batch)
        self.group = group
        self.patch_width = ops.patch_width
        self.render_mode = "clear"
        self.feature_blending_level = 0
        self.rows = self.cols = None
        self.features = self.mask = None
        self._canvas_rank_local, self._sync_layout = False, None
        self.halo_bytes = None
        self.down_factor = None
        self._alpha_cache: Dict[Tuple[int, int, int], torch.Tensor] = {}
        self._noise_set, self._noise_src = None, None       # the brush's noise buffers on the device, and the dict they came from
        self.comm_timing = False                            # record HIP events around the sharded calls' collectives (comm_times)
        self._comm_events: Dict[str, list] = {}

    def _brush_noise(self, opts: "GanBrushOptions"):
        """The noise set of a projected brush: ``opts.custom_args['noise_buffers']`` (what ``formats.WBrushLibrary`` hands to
        ``set_style_w``; the reference renders with ``**opts.custom_args``, brush.py:746-754) as a ``networks.BrushNoise`` that every
        generator pass of the schedule reads.  None -- the checkpoint's noise -- for a z brush, for no / None / empty buffers, and for
        an ``ops`` without noise sets (the CPU stand-ins of the tests).  The helper keeps ONE set and reloads it (one launch on the
        caller's stream, behind the previous call's joined batches) when the dict is another non-empty dict OBJECT than last time:
        a dict changed in place is not seen -- hand ``set_style_w`` a new one.  Every rank of a process group builds its own set
        from the same ``opts``; there is no collective in it."""
        bufs = opts.custom_args.get("noise_buffers") if (opts.style_ws is not None and opts.custom_args) else None
        if not bufs:
            return None
        bn = self._noise_set
        if bn is None or bn.epoch is not bn.syn.packed:       # first brush, or the weights were reloaded / moved since
            bn, self._noise_src = self.ops.brush_noise(), None
            if bn is None:
                return None
            self._noise_set = bn
        if bufs is not self._noise_src:
            bn.load(bufs)
            self._noise_src = bufs
        return bn

    # -- canvas state --
    def make_new_canvas(self, rows: int, cols: int, feature_blending: Optional[int] = None):
        self.rows, self.cols = int(rows), int(cols)
        self.set_feature_blending(self.feature_blending_level if feature_blending is None else feature_blending)

    def set_feature_blending(self, feature_blending_level: int = 0):
        self.feature_blending_level = int(feature_blending_level)
        self.features = self.mask = None
        self._canvas_rank_local, self._sync_layout = False, None
        self.down_factor = 2 ** (self.feature_blending_level - 1) if self.feature_blending_level > 0 else None

    def sync_canvas(self):
        """Make the feature canvas whole on every rank after a sharded ``render_tiles`` (collective: all ranks call it).

        A sharded call replays, on each rank, the paint sequence under that rank's own tiles only (plus the strips of
        earlier foreign tiles under them), so a rank's canvas is final exactly where the LAST tile covering a pixel is one
        of its own.  Every pixel under this call's tiles therefore has one owning rank; the owners' values are summed with
        zeros from everybody else (one all-reduce over the tiles' bounding box: exact, x + 0 + ... + 0) and every rank ends
        up with the canvas the reference's single persistent ``FeatureCanvas`` (brush.py:33-92) would hold.  Runs lazily --
        ``_schedule`` calls it when a second sharded call paints on the same canvas; a canvas that is painted once (the
        ``paint_image`` job) never pays for it."""
        if not self._canvas_rank_local:
            return
        rank, world = self._world()
        rects, bounds = self._sync_layout
        self._canvas_rank_local, self._sync_layout = False, None
        if not self._sharded(world) or self.features is None:
            return
        hc, wc = self.mask.shape
        y0, x0 = max(0, int(rects[:, 0].min())), max(0, int(rects[:, 1].min()))
        y1, x1 = min(hc, int(rects[:, 2].max())), min(wc, int(rects[:, 3].max()))
        if y1 <= y0 or x1 <= x0:
            return
        last = np.full((hc, wc), -1, np.int64)                       # paint order: the last tile over a pixel wins
        owner_of = np.empty(rects.shape[0] + 1, np.int64)
        owner_of[-1] = -1
        for r_, (a, b) in enumerate(bounds):
            owner_of[a:b] = r_
        for t, (a0, b0, a1, b1) in enumerate(rects.tolist()):
            last[max(0, a0):a1, max(0, b0):b1] = t
        owner = owner_of[last[y0:y1, x0:x1]]
        ops = self.ops
        mine = ops.to_device((owner == rank))
        touched = ops.to_device((owner >= 0))
        f = self.features[0, :, y0:y1, x0:x1]
        m = self.mask[y0:y1, x0:x1]
        buf = torch.cat([(f * mine).reshape(-1), (m * mine).to(torch.float32).reshape(-1)])
        dist.all_reduce(buf, op=dist.ReduceOp.SUM, group=self.group)
        nf = f.numel()
        self.features[0, :, y0:y1, x0:x1] = torch.where(touched, buf[:nf].view(f.shape), f)
        self.mask[y0:y1, x0:x1] = torch.where(touched, buf[nf:].view(m.shape).to(torch.uint8), m)

    def set_render_mode(self, mode: str):
        if mode not in ("clear", "full"):
            raise RuntimeError("Unknown render mode for TriadGanPaintEngine: {}".format(mode))
        self.render_mode = mode

    def _alpha0(self, width, margin, crop) -> torch.Tensor:
        key = (width, margin, crop)
        if key not in self._alpha_cache:
            self._alpha_cache[key] = self.ops.to_device(dirty_area_alpha(width, margin, crop))
        return self._alpha_cache[key]

    # -- world --
    def _world(self) -> Tuple[int, int]:
        if dist.is_available() and dist.is_initialized():
            return dist.get_rank(self.group), dist.get_world_size(self.group)
        return 0, 1

    def _sharded(self, world: int) -> bool:
        """Does the call take the multi-rank schedule (halo exchange, pieces replay, tile gather)?  With more than one rank -- or at
        world size 1 under ``NB_FORCE_PG=1`` once the process group exists (launch.py: the very collectives of the N > 1 job, through
        RCCL, on a one-GPU box; same canvases as the single-process schedule)."""
        return world > 1 or (os.environ.get("NB_FORCE_PG") == "1" and dist.is_available() and dist.is_initialized())

    # -- the schedule --
    def _schedule(self, geom_img, geom_yx: np.ndarray, areas_yx: np.ndarray, positions: Optional[np.ndarray],
                  opts: GanBrushOptions, crop_margin: int) -> Optional[torch.Tensor]:
        """Tiles i = 0..T-1 in paint order: geometry cut from ``geom_img`` [H,W] uint8 (255 = background; numpy, or a tensor that
        is on the device already) at
        ``geom_yx[i]``, canvas area at ``areas_yx[i]`` (already floored to the blending grid), noise position
        ``positions[i]`` (None: unshifted noise).  Returns the RGBA tiles [T,R,R,4] uint8 on rank 0 (None elsewhere)
        and leaves the feature canvas updated -- the result of the reference's tile-by-tile loop."""
        ops, df = self.ops, self.down_factor
        job = self._begin_job(geom_img, geom_yx, positions, opts, areas_yx.shape[0])
        if self.feature_blending_level == 0:
            outs = self._render_unblended(job)
        else:
            bres = self.patch_width // df
            C = ops.cfg.channels(bres)
            rects = np.concatenate([areas_yx // df, areas_yx // df + bres], axis=1).astype(np.int64)
            if self.features is None:
                self.features, self.mask = ops.new_feature_canvas(C, -(-self.rows // df), -(-self.cols // df))
            alpha0 = self._alpha0(bres, self.feature_blending_margin // df, crop_margin // df)
            halo = HaloExchange(rects, job.bounds, job.rank, job.world, C, self_probe=job.world == 1) if job.sharded else None
            mine, geom_feats = self._run_heads(job, bres, C, halo)
            self._replay(job, mine, areas_yx // df, rects, alpha0, crop_margin // df, halo)
            outs = self._run_tails(job, mine, geom_feats, bres)
        rgba_own = torch.cat(outs) if outs else None
        return self._gather_tiles(job, rgba_own) if job.sharded else rgba_own

    def _begin_job(self, geom_img, geom_yx, positions, opts: GanBrushOptions, T: int) -> _Job:
        """World split, uploads, the brush (style, noise set, UVS factor) and the stream / slot policy of one call."""
        ops = self.ops
        rank, world = self._world()
        sharded = self._sharded(world)
        if sharded and self.feature_blending_level > 0 and self._canvas_rank_local:
            self.sync_canvas()                   # the previous sharded call left every rank with ITS tiles' paint sequence only
        bounds = [shard_bounds(T, r, world) for r in range(world)]
        t0, t1 = bounds[rank]
        n_own = t1 - t0

        geom_dev = geom_img.contiguous() if torch.is_tensor(geom_img) else ops.to_device(np.ascontiguousarray(geom_img))
        ws1 = ops.map_style(z=opts.style_z, ws=opts.style_ws)                  # one brush style for all tiles
        user = opts.user_colors()
        # a projected brush's noise buffers (the UVS calibration below stays without them, as the reference's: mapper.py:84-87)
        noise_set = self._brush_noise(opts)
        sfac = None
        if opts.enable_uvs_mapping:                                            # brush.py:773-774
            if self.uvs_mapper is None:
                raise RuntimeError("opts.enable_uvs_mapping needs a StyleUVSMapper (PaintingHelper(uvs_mapper=...))")
            sfac = self.uvs_mapper.get_sfactor(opts)
        own_yx = ops.to_device(geom_yx[t0:t1].astype(np.int32)) if n_own else None
        own_pos = ops.to_device(positions[t0:t1].astype(np.int64)) if (positions is not None and n_own) else None

        on_stream, join = ops.stream, ops.join_streams
        # workspace slots of the painting schedule: disjoint from the generator's own sub-batch slots (1..sub_streams), whose
        # side-stream kernels of an un-joined throughput call may still be reading theirs
        # 1 or 2 batch streams: measured, once per TileOps -- by jobs long enough for the ~80 ms probe to be noise (smaller ones keep the
        # default of two: what they could gain or lose is a fraction of a millisecond)
        if n_own >= 6 * self.batch or ops.stream_policy > 0:
            ops.choose_streams(min(self.batch, n_own), self.render_mode)          # (a fixed policy applies to every canvas size)
        plan_slot = lambda k: PAINT_SLOT0 + k % ops.n_streams
        if n_own <= self.batch:                      # a single batch (interactive strokes): nothing to overlap with
            on_stream, join, plan_slot = (lambda k: contextlib.nullcontext()), (lambda tensors=(): None), (lambda k: 0)
        else:
            ops.prepare(min(self.batch, n_own), sorted({plan_slot(k) for k in range(ops.n_streams)}))
        return _Job(rank=rank, world=world, sharded=sharded, T=T, bounds=bounds, t0=t0, t1=t1, geom_dev=geom_dev, ws1=ws1,
                    user_dev=None if user is None else user.to(ops.device), sfac=sfac,
                    nkw={} if noise_set is None else {"noise_set": noise_set}, own_yx=own_yx, own_pos=own_pos,
                    batches=[(b0, min(b0 + self.batch, n_own)) for b0 in range(0, n_own, self.batch)],
                    on_stream=on_stream, join=join, plan_slot=plan_slot)

    def _render_unblended(self, job: _Job) -> List[torch.Tensor]:
        """Level 0: every batch is one full generator pass."""
        ops, outs = self.ops, []
        for k, (b0, b1) in enumerate(job.batches):
            with job.on_stream(k):
                g = ops.geom_tiles(job.geom_dev, job.own_yx[b0:b1])
                outs.append(ops.full(job.style(b1 - b0), ops.encode(g), job.pos(b0, b1), self.render_mode, job.colors(b1 - b0),
                                     job.sfac, slot=job.plan_slot(k), **job.nkw))
        job.join(outs)
        return outs

    def _run_heads(self, job: _Job, bres: int, C: int, halo: Optional[HaloExchange]):
        """Phase 1: everything up to the blending resolution, own tiles -> (``mine`` [n_own,C,bres,bres], the batches' geometry
        features).  The batches run last-to-first: the tiles the later ranks need (the end of my range) finish first, and their
        strips travel under the rest of phase 1.  Returns with the strips of the other ranks received."""
        ops = self.ops
        mine = torch.empty([job.n_own, C, bres, bres], dtype=torch.float32, device=ops.device)
        geom_feats = {}
        for k, (b0, b1) in reversed(list(enumerate(job.batches))):
            with job.on_stream(k):
                gf = ops.encode(ops.geom_tiles(job.geom_dev, job.own_yx[b0:b1]))
                geom_feats[k] = gf
                mine[b0:b1] = ops.head(job.style(b1 - b0), gf, job.pos(b0, b1), bres, slot=job.plan_slot(k), **job.nkw)
            if halo is not None and not halo.started and b0 <= halo.first_send:
                self._start_exchange(halo, mine, job)
        if halo is not None and not halo.started:
            self._start_exchange(halo, mine, job)                                 # (a rank without tiles still takes part)
        job.join()
        if halo is not None:
            # (events on the caller's stream: the first fires when phase 1 is through, the second when the strips are there
            #  -- what of the exchange was NOT hidden under phase 1; comm_times())
            ev = self._comm_event_pair("halo_exchange_exposed_ms")

            def arrived(bufs):
                ops.join_comm(bufs)
                if ev is not None:
                    ev[1].record()
            halo.finish(mine, job.t0, arrived)
        return mine, geom_feats

    def _start_exchange(self, halo: HaloExchange, mine: torch.Tensor, job: _Job) -> None:
        halo.start(mine, job.t0, self.ops.comm_stream, self.group)
        self.halo_bytes = halo.halo_bytes

    def _replay(self, job: _Job, mine, areas, rects, alpha0, crop_sc: int, halo: Optional[HaloExchange]) -> None:
        """Phase 2: the sequential canvas blend of my tiles, replayed in one launch -- over whole tiles, or (sharded) over the
        received strips and my tiles."""
        ops = self.ops
        bres = mine.shape[-1]
        hc, wc = self.mask.shape
        if halo is None:
            off, lst = build_cells(rects, hc, wc)
            # few tiles on a large canvas (interactive strokes): replay only the cells inside their bounding box
            box = None
            if job.T * bres * bres * 4 < hc * wc:
                box = (int(rects[:, 0].min()), int(rects[:, 1].min()), int(rects[:, 2].max()), int(rects[:, 3].max()))
            self.mask = ops.replay(mine, ops.to_device(areas.astype(np.int32)), alpha0, crop_sc,
                                   self.features, self.mask, ops.to_device(off), ops.to_device(lst), **({"box": box} if box else {}))
            return
        if job.n_own:
            pieces, prect = halo.pieces(mine, job.t0, job.t1)
            off, lst = build_cells(np.asarray(prect, np.int64), hc, wc)
            own_r = rects[job.t0:job.t1]
            box = (int(own_r[:, 0].min()), int(own_r[:, 1].min()), int(own_r[:, 2].max()), int(own_r[:, 3].max()))
            self.mask = ops.replay_pieces(pieces, bres, alpha0, crop_sc, self.features, self.mask,
                                          ops.to_device(off), ops.to_device(lst), box)
        # my canvas now holds the paint sequence under MY tiles only; what it takes to make it whole again
        # (sync_canvas, run lazily by the next sharded call on this canvas) is the tile layout of this call
        self._canvas_rank_local = True
        self._sync_layout = (rects.copy(), job.bounds)

    def _run_tails(self, job: _Job, mine, geom_feats, bres: int) -> List[torch.Tensor]:
        """Phase 3: last block(s) + ToRGB + compositing on the blended features, own tiles."""
        ops, outs = self.ops, []
        for k, (b0, b1) in enumerate(job.batches):
            with job.on_stream(k):
                outs.append(ops.tail(job.style(b1 - b0), mine[b0:b1], geom_feats[k], job.pos(b0, b1), bres,
                                     self.render_mode, job.colors(b1 - b0), job.sfac, slot=job.plan_slot(k), **job.nkw))
        job.join(outs)
        return outs

    def _gather_tiles(self, job: _Job, rgba_own: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
        """The ranks' RGBA tiles on rank 0, in paint order (None elsewhere): one gather of equally padded buffers."""
        R, world = self.patch_width, job.world
        buf = torch.zeros([-(-job.T // world), R, R, 4], dtype=torch.uint8, device=self.ops.device)
        if job.n_own:
            buf[:job.n_own] = rgba_own
        recv = [torch.empty_like(buf) for _ in range(world)] if job.rank == 0 else None
        ev = self._comm_event_pair("tile_gather_ms")
        dist.gather(buf, recv, dst=0, group=self.group)
        if ev is not None:
            ev[1].record()
        if job.rank != 0:
            return None
        return torch.cat([recv[r][:n] for r, n in enumerate(shard_sizes(job.T, world))])

    def _comm_event_pair(self, name: str):
        """A pair of HIP events around a collective of the sharded schedule (first one recorded here, on the caller's stream).
        Only when ``self.comm_timing`` is set (benchmarks: tools/bench_canvas.py): the product path records nothing."""
        if not self.comm_timing or self.ops.device.type != "cuda":
            return None
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        self._comm_events.setdefault(name, []).append((e0, e1))
        return e0, e1

    def comm_times(self, reset: bool = True) -> Dict[str, float]:
        """Milliseconds this rank's stream spent on the collectives of the sharded calls since the last reset: the part of the
        halo exchange that phase 1 did not hide, and the gather of the RGBA tiles on rank 0 (synchronises the device)."""
        evs = self._comm_events
        if not evs:
            return {}
        torch.cuda.synchronize(self.ops.device)
        out = {k: round(sum(a.elapsed_time(b) for a, b in v), 4) for k, v in evs.items()}
        out["calls"] = max(len(v) for v in evs.values())
        if reset:
            self._comm_events = {}
        return out

    def render_tiles(self, geom_padded, crops: Sequence[Tuple[int, int]], opts: GanBrushOptions,
                     crop_margin: int = 0, out_canvas: Optional[torch.Tensor] = None):
        """Render the tiles whose top-left corners (y, x) are ``crops`` from the padded geometry [H,W] uint8
        (255 = background; numpy or a device tensor) and paste them into ``out_canvas`` [H,W,4] uint8 on the device (rank 0; created if None).
        Equivalent to calling the reference's ``render_stroke`` on the tiles in order with
        ``opts.set_position(x, y)`` (paint_image_main.py:157-177).  Returns the canvas on rank 0, None elsewhere."""
        ops, R = self.ops, self.patch_width
        H, W = geom_padded.shape[:2]
        if self.rows is None:
            self.make_new_canvas(H, W)
        crops = np.asarray([c[:2] for c in crops], np.int64).reshape(-1, 2)
        if crops.shape[0] == 0:
            raise ValueError("no tiles to render")
        df = self.down_factor
        floored = crops if self.feature_blending_level == 0 else (crops // df) * df      # brush.py:253-258
        rgba_all = self._schedule(geom_padded.reshape(H, W), crops, floored, crops, opts, crop_margin)
        if rgba_all is None:
            return None
        if out_canvas is None:
            out_canvas = torch.zeros([H, W, 4], dtype=torch.uint8, device=ops.device)
        m = int(crop_margin)
        off, lst = build_cells(np.concatenate([floored + m, floored + R - m], axis=1), H, W)
        ops.paste(out_canvas, rgba_all, ops.to_device(floored.astype(np.int32)), m, ops.to_device(off), ops.to_device(lst))
        return out_canvas

    graph_strokes = True       # render_stroke replays hipGraph-captured generator passes (TileOps.graph_single)

    def render_stroke(self, stroke_patch: np.ndarray, canvas_patch, opts: GanBrushOptions, meta: Optional[dict] = None):
        """One R x R tile (reference contract, brush.py:244-398): ``stroke_patch`` [R,R,1|4] uint8 with opaque 255 =
        stroke; returns (RGBA uint8 [R-2m, R-2m, 4] numpy, None, {'x','y'}) and updates the feature canvas.
        Single-process call (interactive sessions are one GPU each)."""
        R = self.patch_width
        H, W, _ = stroke_patch.shape
        if W != R or H != R:
            raise RuntimeError("Not implemented")                                  # as the reference, brush.py:273-274
        x = y = m = 0
        if meta is not None:
            x, y = int(meta.get("x")), int(meta.get("y"))
            m = int(meta.get("crop_margin", 0))
        if self.feature_blending_level > 0:
            assert meta is not None, "feature blending needs the tile position"     # brush.py:303
            assert self.rows is not None, "Must call make_new_canvas before rendering with feature blending"
        df = self.down_factor or 1
        fy, fx = (y // df) * df, (x // df) * df
        geom = (255 - stroke_patch[:, :, -1]).astype(np.uint8)                     # back to 255 = background
        pos = None if opts.position is None else opts.position.numpy().reshape(1, 2)
        prev = self.ops.graph_single
        if prev is not None and self.graph_strokes:
            self.ops.graph_single = True                  # one tile per call: replay captured generator passes
        try:
            rgba = self._schedule(geom, np.zeros((1, 2), np.int64), np.array([[fy, fx]], np.int64), pos, opts, m)
        finally:
            if prev is not None:
                self.ops.graph_single = prev
        img = rgba[0, m:R - m, m:R - m].cpu().numpy()
        return np.ascontiguousarray(img), None, {"x": fx + m, "y": fy + m}

    def paint_image(self, geom: np.ndarray, opts: GanBrushOptions, crop_margin: int = 10, stitching_mode: str = "all",
                    on_white: bool = False, return_full: bool = False):
        """``paint_image_main.py:145-192`` from the thresholded geometry image [H,W,1] uint8 (255 = background):
        pad, tile with 2*crop_margin overlap, stylize every tile, paste, composite, crop.  Rank 0 returns the image."""
        geom = np.asarray(geom, np.uint8)
        if geom.ndim == 2:
            geom = geom[..., None]
        R = self.patch_width
        padded0 = pad_geo(geom, crop_margin)
        crops, padded = generate_stitching_crops(padded0, R, mode=stitching_mode, overlap_margin=2 * crop_margin)
        self.make_new_canvas(padded.shape[0], padded.shape[1], self.feature_blending_level)
        canvas = self.render_tiles(padded[..., 0], crops, opts, crop_margin=crop_margin)
        if canvas is None:
            return None
        m, (h0, w0) = crop_margin, geom.shape[:2]
        to_host = self.ops.to_host
        result = canvas[m:m + h0, m:m + w0]                          # crop on the device: only the answer crosses PCIe
        if on_white:
            result = _on_white_torch(self.ops, result)
        out = to_host(result.contiguous())
        if not return_full:
            return out
        return out, to_host(canvas), crops, padded

    def paint_drawing(self, img: np.ndarray, opts: GanBrushOptions, crop_margin: int = 10, stitching_mode: str = "all",
                      on_white: bool = False, return_full: bool = False):
        """``paint_image(prepare_geometry_image(img), ...)`` with the preparation on the device: the decoded drawing (uint8 [H,W],
        [H,W,3] or [H,W,4]) is uploaded once, thresholded straight into the padded geometry (``nb_geom_prepare_u8``), the tiles are
        picked from per-tile stroke counts (``nb_tile_stroke_counts_u8``), the schedule runs on the device-resident geometry and the
        result is cropped / composited on white on the device.  Same bytes as the host route.  An ``ops`` without the preparation
        kernels (the CPU stand-ins of the tests) takes the numpy helpers."""
        ops, R, m = self.ops, self.patch_width, int(crop_margin)
        if not all(hasattr(ops, k) for k in ("prepare_geometry", "stroke_counts", "composite_on_white")):
            return self.paint_image(prepare_geometry_image(img), opts, crop_margin=crop_margin, stitching_mode=stitching_mode,
                                    on_white=on_white, return_full=return_full)
        img = np.asarray(img)
        if img.dtype != np.uint8 or img.ndim not in (2, 3) or (img.ndim == 3 and img.shape[2] not in (1, 3, 4)):
            raise ValueError(f"paint_drawing: uint8 [H,W], [H,W,3] or [H,W,4] expected, got {img.dtype} {img.shape}")
        h0, w0 = img.shape[:2]
        nrows, ncols, stride, ph, pw = stitching_grid(h0 + m, w0 + m, R, 2 * m)
        padded = ops.prepare_geometry(img, (ph, pw), (m, m))
        return self._paint_padded(padded, (h0, w0), (nrows, ncols, stride), opts, m, stitching_mode, on_white, return_full)

    def _paint_padded(self, padded: torch.Tensor, size_hw, grid, opts: GanBrushOptions, m: int, stitching_mode: str, on_white: bool,
                      return_full: bool):
        """The device route behind the padded geometry [ph, pw] uint8 (the drawing at (m, m), 255 around it): tile picks, the
        schedule, crop / composite on white."""
        ops, R = self.ops, self.patch_width
        (h0, w0), (nrows, ncols, stride), (ph, pw) = size_hw, grid, padded.shape
        if stitching_mode == "all":
            keep = np.ones((nrows, ncols), bool)
        else:
            keep = ops.to_host(ops.stroke_counts(padded, R, stride, nrows, ncols)) > 10
        crops = [(int(r) * stride, int(c) * stride, R, R) for r, c in zip(*np.nonzero(keep))]       # row-major, as the host loop
        self.make_new_canvas(ph, pw, self.feature_blending_level)
        canvas = self.render_tiles(padded, crops, opts, crop_margin=m)
        if canvas is None:
            return None
        if on_white:
            result = ops.composite_on_white(canvas, m, m, h0, w0)
        else:
            result = canvas[m:m + h0, m:m + w0].contiguous()
        out = ops.to_host(result)
        if not return_full:
            return out
        return out, ops.to_host(canvas), crops, ops.to_host(padded)[..., None]

    def paint_strokes(self, strokes: StrokeList, size_hw, opts: GanBrushOptions, crop_margin: int = 10, stitching_mode: str = "all",
                      on_white: bool = False, return_full: bool = False, subdiv: int = 8):
        """``paint_drawing`` from strokes instead of a raster: the strokes of a [h, w] = ``size_hw`` drawing (``StrokeList``: points and
        radii, kilobytes) are uploaded, splines are cut into segments and all segments rasterised straight into the padded geometry on
        the device (``nb_spline_flatten_f32``, ``nb_raster_segments_u8``); tile picks, schedule, crop and on-white follow as in
        ``paint_drawing``.  Strokes are clipped to the drawing: the padding around it stays background.  Same bytes as
        ``paint_image`` on the rasterised strokes.  An ``ops`` without the kernels (the CPU stand-ins of the tests) takes the numpy
        restatement.  Every rank of a sharded run rasterises the stroke list itself."""
        ops, R, m = self.ops, self.patch_width, int(crop_margin)
        h0, w0 = int(size_hw[0]), int(size_hw[1])
        if h0 < 1 or w0 < 1:
            raise ValueError(f"paint_strokes: bad canvas size {size_hw}")
        if not all(hasattr(ops, k) for k in ("raster_strokes", "stroke_counts", "composite_on_white")):
            return self.paint_image(raster_strokes_numpy(strokes, (h0, w0), (0, 0), subdiv), opts, crop_margin=crop_margin,
                                    stitching_mode=stitching_mode, on_white=on_white, return_full=return_full)
        nrows, ncols, stride, ph, pw = stitching_grid(h0 + m, w0 + m, R, 2 * m)
        padded = ops.raster_strokes(strokes, (ph, pw), (m, m), subdiv=subdiv)
        padded[:m].fill_(255)                                 # the padding is background, whatever the strokes reach
        padded[m + h0:].fill_(255)
        padded[:, :m].fill_(255)
        padded[:, m + w0:].fill_(255)
        return self._paint_padded(padded, (h0, w0), (nrows, ncols, stride), opts, m, stitching_mode, on_white, return_full)


# ------------------------------------------------------------------------------------------------
# the paint session: a canvas that stays on the device, strokes added one call at a time, each with its own brush
# ------------------------------------------------------------------------------------------------
EMPTY_BOX = (0, 0, 0, 0)


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


class PaintSession:
    """What a paint program does with the engine: a RGBA canvas that stays on the device, onto which every ``add`` renders a few
    strokes with their own brush and colours and composites them over (or erases with them) what is already there.  Only the tiles the
    strokes touch are rendered, and the caller fetches only what it wants to look at (``view``, ``image``).

    The canvas has the frame of ``paint_strokes``: the padded size of ``stitching_grid(h0 + m, w0 + m, R, 2 m)`` with the drawing at
    (m, m), so tiles sit on the same grid and get the same noise positions, and one ``add`` on an empty canvas leaves what
    ``paint_strokes(..., stitching_mode="stroke")`` paints.  Feature blending works among the tiles of one call; the reference's one
    feature canvas across all strokes of a session remains what ``render_stroke`` offers.  Single process, like ``render_stroke``.

    In the reference this is split between the server (rendering) and the browser client, which writes the returned patches into a
    foreground layer and draws that layer over the background canvas when the stroke ends (main_controller.js:776, 131-141)."""

    def __init__(self, helper: "PaintingHelper", size_hw, crop_margin: int = 10, undo_depth: int = 8):
        import collections
        _, world = helper._world()
        if helper._sharded(world):
            raise RuntimeError("PaintSession runs in a single process (a sharded helper paints whole drawings: paint_strokes)")
        h0, w0, m = int(size_hw[0]), int(size_hw[1]), int(crop_margin)
        if h0 < 1 or w0 < 1 or m < 0 or int(undo_depth) < 0:
            raise ValueError(f"PaintSession: bad size {size_hw}, crop margin {crop_margin} or undo depth {undo_depth}")
        self.helper, self.ops, self.size_hw, self.crop_margin = helper, helper.ops, (h0, w0), m
        self.grid = stitching_grid(h0 + m, w0 + m, helper.patch_width, 2 * m)       # (nrows, ncols, stride, padded_h, padded_w)
        ph, pw = self.grid[3:]
        self.canvas = torch.zeros([ph, pw, 4], dtype=torch.uint8, device=self.ops.device)
        helper.make_new_canvas(ph, pw)
        self._undo = collections.deque(maxlen=int(undo_depth))                      # (canvas box, the bytes it held)
        self._mask_seen, self._mask_rect = None, None                               # the helper's feature mask as the last add left it
        self.last_tiles = 0                                                         # tiles the last add rendered

    def _drawing_box(self, box) -> Tuple[int, int, int, int]:
        """A canvas box in drawing coordinates, clipped to the drawing."""
        m, (h0, w0) = self.crop_margin, self.size_hw
        y0, x0, y1, x1 = max(0, box[0] - m), max(0, box[1] - m), min(h0, box[2] - m), min(w0, box[3] - m)
        return (y0, x0, y1, x1) if y1 > y0 and x1 > x0 else EMPTY_BOX

    def _reset_feature_mask(self) -> None:
        """Feature blending is per call: un-set the feature mask where the previous add set it.  The features stay -- the replay never
        reads a feature whose mask bit is 0 -- and so does the allocation."""
        helper = self.helper
        ph, pw = self.grid[3:]
        if (helper.rows, helper.cols) != (ph, pw):              # the helper has painted something else in between
            helper.make_new_canvas(ph, pw)
        elif helper.mask is not None:
            if helper.mask is self._mask_seen and self._mask_rect is not None:
                y0, x0, y1, x1 = self._mask_rect
                helper.mask[y0:y1, x0:x1].zero_()
            else:
                helper.mask.zero_()
        self._mask_seen = self._mask_rect = None

    def add(self, strokes: StrokeList, opts: GanBrushOptions, mode: str = "paint", opacity: int = 255, subdiv: int = 8):
        """Render ``strokes`` with the brush of ``opts`` and composite them into the canvas: ``mode`` "paint" (source-over) or "erase"
        (destination-out by the rendered strokes' alpha), ``opacity`` 0..255 on top of the strokes' own alpha.  Returns the dirty box
        (y0, x0, y1, x1), end-exclusive, in drawing coordinates; a call that renders no tile (strokes outside the drawing, or at most
        10 stroke pixels per tile) changes nothing, saves no undo entry and returns ``EMPTY_BOX``."""
        if mode not in COMPOSE_MODES:
            raise ValueError(f"PaintSession.add: mode {mode!r} is neither 'paint' nor 'erase'")
        if int(opacity) != opacity or not 0 <= int(opacity) <= 255:
            raise ValueError(f"PaintSession.add: opacity {opacity!r} outside 0..255")
        helper, ops, R, m = self.helper, self.ops, self.helper.patch_width, self.crop_margin
        (h0, w0), (nrows, ncols, stride, ph, pw) = self.size_hw, self.grid
        self.last_tiles = 0
        bounds = strokes_bounds(strokes, subdiv)
        if bounds is None:
            return EMPTY_BOX
        by0, bx0, by1, bx1 = max(0, bounds[0]), max(0, bounds[1]), min(h0, bounds[2]), min(w0, bounds[3])
        if by1 <= by0 or bx1 <= bx0:
            return EMPTY_BOX
        # the tiles of the stitching grid whose window [row * stride, row * stride + R) meets the box (canvas = drawing + m)
        r0, r1 = max(0, -(-(by0 + m - R + 1) // stride)), min(nrows - 1, (by1 + m - 1) // stride)
        c0, c1 = max(0, -(-(bx0 + m - R + 1) // stride)), min(ncols - 1, (bx1 + m - 1) // stride)
        nr, nc, gy0, gx0 = r1 - r0 + 1, c1 - c0 + 1, r0 * stride, c0 * stride
        # this call's strokes alone, in a scratch geometry over just those tiles; the padding around the drawing stays background
        sh, sw = (nr - 1) * stride + R, (nc - 1) * stride + R
        top, bottom = min(sh, max(0, m - gy0)), min(sh, max(0, m + h0 - gy0))
        left, right = min(sw, max(0, m - gx0)), min(sw, max(0, m + w0 - gx0))
        if hasattr(ops, "raster_strokes") and hasattr(ops, "stroke_counts"):
            geom = ops.raster_strokes(strokes, (sh, sw), (m - gy0, m - gx0), subdiv=subdiv)
            for pad in (geom[:top], geom[bottom:], geom[:, :left], geom[:, right:]):
                pad.fill_(255)
            counts = ops.to_host(ops.stroke_counts(geom, R, stride, nr, nc))
        else:
            g = raster_strokes_numpy(strokes, (sh, sw), (m - gy0, m - gx0), subdiv)
            for pad in (g[:top], g[bottom:], g[:, :left], g[:, right:]):
                pad[...] = 255
            counts = np.array([[int((g[r * stride:r * stride + R, c * stride:c * stride + R] == 0).sum()) for c in range(nc)]
                               for r in range(nr)])
            geom = ops.to_device(g)
        geom_yx = np.argwhere(counts > 10).astype(np.int64) * stride       # row-major: the order of generate_stitching_crops
        if geom_yx.shape[0] == 0:
            return EMPTY_BOX
        self.last_tiles = geom_yx.shape[0]
        crops = geom_yx + np.array([gy0, gx0], np.int64)
        df = helper.down_factor
        floored = crops if helper.feature_blending_level == 0 else (crops // df) * df
        self._reset_feature_mask()
        rgba = helper._schedule(geom, geom_yx, floored, crops, opts, m)
        if helper.feature_blending_level > 0:
            a, bres = floored // df, R // df
            self._mask_seen = helper.mask
            self._mask_rect = (int(a[:, 0].min()), int(a[:, 1].min()), int(a[:, 0].max()) + bres, int(a[:, 1].max()) + bres)
        rects = np.concatenate([floored + m, floored + R - m], axis=1)     # the interiors: what the paste of render_tiles writes
        box = (max(0, int(rects[:, 0].min())), max(0, int(rects[:, 1].min())), min(ph, int(rects[:, 2].max())), min(pw, int(rects[:, 3].max())))
        self._undo.append((box, self.canvas[box[0]:box[2], box[1]:box[3]].clone()))
        off, lst = build_cells(rects, ph, pw)
        ops.over_tiles(self.canvas, rgba, ops.to_device(floored.astype(np.int32)), m, ops.to_device(off), ops.to_device(lst), box=box,
                       mode=COMPOSE_MODES[mode], opacity=int(opacity))
        return self._drawing_box(box)

    def undo(self) -> Tuple[int, int, int, int]:
        """Put back what the last ``add`` that is still remembered (``undo_depth``) painted over; returns its dirty box, ``EMPTY_BOX``
        when there is nothing to undo."""
        if not self._undo:
            return EMPTY_BOX
        box, saved = self._undo.pop()
        self.canvas[box[0]:box[2], box[1]:box[3]].copy_(saved)
        return self._drawing_box(box)

    def view(self, box=None, k: int = 1, on_white: bool = False) -> np.ndarray:
        """The part (y0, x0, y1, x1) of the drawing (None: all of it) reduced by the integer factor ``k`` in 1..16, as numpy
        [ceil(h/k), ceil(w/k), 4] RGBA or [.., 3] over white: alpha-weighted means (``canvas_view``).  The preview path -- only the
        reduced window crosses PCIe; ``image`` is the exported result."""
        m, (h0, w0) = self.crop_margin, self.size_hw
        y0, x0, y1, x1 = (0, 0, h0, w0) if box is None else (max(0, int(box[0])), max(0, int(box[1])), min(h0, int(box[2])), min(w0, int(box[3])))
        if y1 <= y0 or x1 <= x0:
            raise ValueError(f"PaintSession.view: the box {box} misses the {h0} x {w0} drawing")
        return self.ops.to_host(self.ops.canvas_view(self.canvas, y0 + m, x0 + m, y1 - y0, x1 - x0, k, on_white))

    def image(self, on_white: bool = False) -> np.ndarray:
        """The drawing-sized result, as ``paint_strokes`` returns it: [h0, w0, 4] RGBA, or [h0, w0, 3] composited on white."""
        ops, m, (h0, w0) = self.ops, self.crop_margin, self.size_hw
        if not on_white:
            return ops.to_host(self.canvas[m:m + h0, m:m + w0].contiguous())
        if hasattr(ops, "composite_on_white"):
            return ops.to_host(ops.composite_on_white(self.canvas, m, m, h0, w0))
        return ops.to_host(_on_white_torch(ops, self.canvas[m:m + h0, m:m + w0]))
