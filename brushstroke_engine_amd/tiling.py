"""Host-side geometry and tiling of the painting engine (numpy; no device work, nothing of ``strokes``, ``tile_ops`` or ``painting``).

What the reference does on the host around its tile loop -- ``_read_any_geo`` and ``pad_geo`` (``forger/viz/paint_image_main.py:30-61``),
``generate_stitching_crops`` (``forger/viz/style_transfer.py:15-48``), ``generate_dirty_area_alpha`` (``forger/ui/brush.py:159-187``) --
and this build's own bookkeeping of a call's tiles: which tiles a drawing needs, where they land on the canvas, and the per-cell
tile lists of include/neube_hip.h ("Cells") that the canvas kernels walk."""
from __future__ import annotations

import ctypes as C
import dataclasses
from typing import Optional, Tuple

import numpy as np

from . import _lib

CELL_H, CELL_W = 4, 64          # NB_CELL_H / NB_CELL_W of include/neube_hip.h


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


def clear_outside(geom, top: int, bottom: int, left: int, right: int) -> None:
    """Everything of the geometry tensor ``geom`` [H,W] uint8 (host or device) outside rows [top, bottom) and columns [left, right)
    -- the drawing's window, which may reach past the buffer -- becomes background (255), in place: the padding around a drawing
    stays background, whatever the strokes reach."""
    h, w = geom.shape
    top, bottom, left, right = min(h, max(0, top)), min(h, max(0, bottom)), min(w, max(0, left)), min(w, max(0, right))
    for pad in (geom[:top], geom[bottom:], geom[:, :left], geom[:, right:]):
        pad.fill_(255)


def tiles_with_strokes(counts: np.ndarray, stride: int) -> np.ndarray:
    """[T, 2] int64 corners (y, x) of the tiles of a stitching grid that hold more than 10 stroke pixels (``counts`` [nrows, ncols]:
    stroke pixels per tile), row-major: the ``mode != "all"`` rule and the order of ``generate_stitching_crops``."""
    return np.argwhere(np.asarray(counts) > 10).astype(np.int64) * int(stride)


@dataclasses.dataclass(frozen=True)
class TileLayout:
    """Where the tiles of one call land on the canvas: ``floored`` [T, 2], their corners moved down to the blending grid (brush.py:253-258;
    the corners themselves at level 0), and ``rects`` [T, 4], the interiors ``[floored + m, floored + r - m)`` that ``paste`` and
    ``over_tiles`` write."""
    floored: np.ndarray
    rects: np.ndarray
    m: int

    @classmethod
    def of(cls, crops: np.ndarray, r: int, m: int, down_factor: Optional[int]) -> "TileLayout":
        floored = crops if not down_factor else (crops // down_factor) * down_factor
        return cls(floored, np.concatenate([floored + m, floored + r - m], axis=1), int(m))

    def box(self, h: int, w: int) -> Tuple[int, int, int, int]:
        """(y0, x0, y1, x1) around all interiors, clipped to the h x w canvas."""
        r = self.rects
        return max(0, int(r[:, 0].min())), max(0, int(r[:, 1].min())), min(h, int(r[:, 2].max())), min(w, int(r[:, 3].max()))

    def device_args(self, to_device, h: int, w: int) -> tuple:
        """(dst_yx, crop, cell_off, cell_tiles): what ``paste`` / ``over_tiles`` take after the canvas and the tiles, the arrays
        uploaded with ``to_device`` (corners first, then the cell lists of the interiors on the h x w canvas)."""
        off, lst = build_cells(self.rects, h, w)
        return to_device(self.floored.astype(np.int32)), self.m, to_device(off), to_device(lst)
