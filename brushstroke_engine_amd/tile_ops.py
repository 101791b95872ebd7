"""The device operations of the painting engine, as the drivers of ``painting`` see them (imports ``tiling`` and ``strokes``, nothing of
``painting``).

``TileOps`` is the product: the HIP generator split in two, the PyTorch-ROCm geometry encoder, and the canvas, preparation,
compositing and stroke kernels.  ``TileOpsBase`` is what it derives from, and what the CPU stand-ins of the tests derive from: the
scheduling hooks with defaults that do nothing, and a host restatement (numpy or torch, also in this module) of every operation
that has one.  The drivers call ``ops.<operation>`` and never ask which ops they hold; a missing kernel is an error, not a fallback."""
from __future__ import annotations

import contextlib
import dataclasses
import inspect
import os
import time
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib
from .strokes import SEG_PITCH, StrokeList, raster_strokes_numpy
from .tiling import CELL_H, CELL_W, cell_box, prepare_geometry_image

PAINT_SLOT0 = 8                 # first generator workspace slot of the tiled schedule (TileOps._GRAPH_SLOT = 16 onwards: graphs)

# ------------------------------------------------------------------------------------------------
# compositing (csrc/nb_compose.hip): the two contracts of include/neube_hip.h restated in int64
# ------------------------------------------------------------------------------------------------
COMPOSE_MODES = {"paint": 0, "erase": 1}


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


def stroke_counts_numpy(geom: np.ndarray, r: int, stride: int, nrows: int, ncols: int) -> np.ndarray:
    """``nb_tile_stroke_counts_u8`` in numpy: [nrows, ncols] int32, the stroke pixels (bytes == 0) of ``geom`` [H,W] uint8 in the
    r x r window at (row * stride, col * stride) of every tile; what of a window lies outside the image counts nothing."""
    stroke = np.asarray(geom) == 0
    return np.array([[stroke[y:y + r, x:x + r].sum() for x in range(0, ncols * stride, stride)]
                     for y in range(0, nrows * stride, stride)], np.int32).reshape(nrows, ncols)


def on_white_torch(rgba: torch.Tensor) -> torch.Tensor:
    """paint_image_main.py:179-183 as a torch expression (3 channels out), on the device of ``rgba``: what
    ``nb_composite_on_white_u8`` computes.  The host route ``PaintingHelper.paint_image`` and ``TileOpsBase`` use it."""
    # alpha = a / 255 through a host-computed table: device division is not correctly rounded
    lut = torch.from_numpy(np.arange(256, dtype=np.float32) / np.float32(255)).to(rgba.device, non_blocking=True)
    a = lut[rgba[..., 3:].to(torch.int64)]
    return (rgba[..., :3].to(torch.float32) * a + 255 * (1 - a)).clip(0, 255).to(torch.uint8)


# ------------------------------------------------------------------------------------------------
# device operations (HIP)
# ------------------------------------------------------------------------------------------------
def _p(t):
    return None if t is None else t.data_ptr()


def _select_shapes(x: torch.Tensor, mask: torch.Tensor, k: int) -> Tuple[int, int, int]:
    """(n, count, m) of a ``masked_kth_largest`` call, or ValueError."""
    if x.dtype != torch.float32 or x.dim() not in (3, 4) or (x.dim() == 4 and x.shape[1] != 1) or x.shape[0] < 1:
        raise ValueError(f"masked_kth_largest: float32 [n,1,h,w] or [n,h,w] expected, got {x.dtype} {tuple(x.shape)}")
    n, count = x.shape[0], x.shape[-2] * x.shape[-1]
    if mask.dtype not in (torch.bool, torch.uint8) or mask.dim() < 1 or mask.shape[0] < 1 or mask.numel() != mask.shape[0] * count:
        raise ValueError(f"masked_kth_largest: bool / uint8 masks [m, ...] of {count} elements each expected, got {mask.dtype} "
                         f"{tuple(mask.shape)}")
    if int(k) < 1 or count < 1:
        raise ValueError(f"masked_kth_largest: k = {k} and {count} elements per image: both must be at least 1")
    return n, count, mask.shape[0]


# ------------------------------------------------------------------------------------------------
# brush scores (csrc/nb_metrics.hip): the reference's own operations, in its order, in float32 torch
# ------------------------------------------------------------------------------------------------
BG_THRESH, FG_THRESH = 0.999, 0.3          # compute_transparency_metrics (forger/metrics/geom_metric.py:156-157)


@dataclasses.dataclass
class EvalMasks:
    """What ``eval_masks`` leaves for ``brush_metrics``, where the drawings are."""
    geom: torch.Tensor               # [K,R,R] float32, 0 = stroke
    blur: torch.Tensor               # [K,R,R] float32: the 5x5 Gaussian applied twice, zero padding at each application
    mask: torch.Tensor               # [K,R,R] uint8: bit 0 = background (blur > 0.999), bit 1 = foreground (geom < 0.3)
    n_bg: torch.Tensor               # [K] int32
    n_fg: torch.Tensor               # [K] int32


def gaussian_blur_torch(img: torch.Tensor) -> torch.Tensor:
    """``default_gaussian_smoothing`` (geom_metric.py:73-129) on [n,1,h,w]: 5x5, sigma 1, normalised, zero padding 2."""
    ax = torch.arange(5, dtype=torch.float32)
    g = 1 / (1 * np.sqrt(2 * np.pi)) * torch.exp(-((ax - 2) / 1) ** 2 / 2)
    kernel = g[:, None] * g[None, :]
    kernel = (kernel / torch.sum(kernel)).view(1, 1, 5, 5).to(img.device)
    return torch.nn.functional.conv2d(img, kernel, padding=2)


def rgb2lab_torch(srgb: torch.Tensor) -> torch.Tensor:
    """``rgb2lab`` (forger/util/color.py:52-140) on [..., 3] in the dtype of ``srgb``, operation by operation."""
    t, dev = srgb.dtype, srgb.device
    lin = (srgb / 12.92 * (srgb <= 0.04045).to(t)) + (((srgb + 0.055) / 1.055) ** 2.4) * (srgb > 0.04045).to(t)
    xyz = torch.matmul(lin, torch.tensor([[0.412453, 0.212671, 0.019334], [0.357580, 0.715160, 0.119193],
                                          [0.180423, 0.072169, 0.950227]], dtype=t, device=dev))
    xyz = xyz * torch.tensor([1.0 / 0.95047, 1.0, 1.0 / 1.08883], dtype=t, device=dev)
    delta = 6.0 / 29.0
    f = (xyz * (1.0 / (3 * delta ** 2)) + 4.0 / 29) * (xyz < delta ** 3.0).to(t) + torch.pow(xyz + 1.0e-8, 1.0 / 3.0) * (xyz >= delta ** 3.0).to(t)
    return torch.matmul(f, torch.tensor([[0.0, 500.0, 0.0], [116.0, -500.0, 200.0], [0.0, 0.0, -200.0]], dtype=t, device=dev)) + \
        torch.tensor([-16.0, 0.0, 0.0], dtype=t, device=dev)


def lab_deltas_torch(target_rgb: torch.Tensor, renders: torch.Tensor, ignore_transparency: bool = False) -> torch.Tensor:
    """``compute_lab_deltas`` (forger/metrics/color_metric.py:29-49): [n,R,R] Lab distance of every pixel to its image's target."""
    if ignore_transparency:
        rgb = renders[:, :3]
    else:
        alpha = renders[:, 3].unsqueeze(1)
        rgb = alpha * renders[:, :3] + (1 - alpha) * 1.0
    lab = rgb2lab_torch(rgb.permute(0, 2, 3, 1).reshape(-1, 3)).reshape(rgb.shape[0], rgb.shape[2], rgb.shape[3], 3).permute(0, 3, 1, 2)
    return torch.linalg.norm(lab - rgb2lab_torch(target_rgb).unsqueeze(-1).unsqueeze(-1), dim=1)


def _metric_shapes(renders: torch.Tensor, target_rgb: torch.Tensor, masks: EvalMasks) -> Tuple[int, int, int]:
    """(n, K, R) of a ``brush_metrics`` call, or ValueError."""
    if renders.dtype != torch.float32 or renders.dim() != 4 or renders.shape[1] != 4 or renders.shape[2] != renders.shape[3]:
        raise ValueError(f"brush_metrics: float32 renders [n,4,R,R] expected, got {renders.dtype} {tuple(renders.shape)}")
    n, r = renders.shape[0], renders.shape[2]
    if target_rgb.dtype != torch.float32 or tuple(target_rgb.shape) != (n, 3):
        raise ValueError(f"brush_metrics: float32 target colours [{n},3] expected, got {target_rgb.dtype} {tuple(target_rgb.shape)}")
    if masks.geom.dim() != 3 or masks.geom.shape[0] < 1 or tuple(masks.geom.shape[1:]) != (r, r):
        raise ValueError(f"brush_metrics: masks of [K,{r},{r}] drawings expected, got {tuple(masks.geom.shape)}")
    return n, masks.geom.shape[0], r


BG_THRESH_PATCHES = 0.99                   # compute_uniform_bg_lpips_metric (geom_metric.py:238), on the guidance blurred ONCE


@dataclasses.dataclass
class BgGuidance:
    """What ``bg_guidance`` leaves for ``bg_mean_colors`` and ``metric_pairs``, where the drawings are."""
    geom: torch.Tensor               # [K,R,R] float32, 0 = stroke
    blur1: torch.Tensor              # [K,R,R] float32: the 5x5 Gaussian applied once, zero padding
    n_bg: torch.Tensor               # [K] int32: pixels with blur1 > 0.99


def _render_shapes(what: str, renders: torch.Tensor, guidance: Optional[BgGuidance]) -> Tuple[int, int, int]:
    """(n, K, R) of a ``bg_mean_colors`` / ``metric_pairs`` call (K = 1 without a guidance), or ValueError."""
    if renders.dtype != torch.float32 or renders.dim() != 4 or renders.shape[1] != 4 or renders.shape[2] != renders.shape[3]:
        raise ValueError(f"{what}: float32 renders [n,4,R,R] expected, got {renders.dtype} {tuple(renders.shape)}")
    n, r = renders.shape[0], renders.shape[2]
    if guidance is None:
        return n, 1, r
    g = guidance.blur1
    if g.dtype != torch.float32 or g.dim() != 3 or g.shape[0] < 1 or tuple(g.shape[1:]) != (r, r) or tuple(guidance.n_bg.shape) != (g.shape[0],):
        raise ValueError(f"{what}: the guidance of [K,{r},{r}] drawings expected, got blur1 {tuple(g.shape)}, n_bg {tuple(guidance.n_bg.shape)}")
    return n, g.shape[0], r


def _pair_shapes(renders, guidance, mean, off0, off1, src1, p, masked) -> Tuple[int, int, int]:
    """(n, K, R) of a ``metric_pairs`` call, or ValueError."""
    n, k, r = _render_shapes("metric_pairs", renders, guidance if masked else None)
    if not 1 <= int(p) <= r:
        raise ValueError(f"metric_pairs: patch width {p} outside 1..{r}")
    for name, off in (("off0", off0), ("off1", off1)):
        if off.dtype != torch.int32 or tuple(off.shape) != (n, 2):
            raise ValueError(f"metric_pairs: int32 {name} [{n},2] expected, got {off.dtype} {tuple(off.shape)}")
    if src1 is not None and (src1.dtype != torch.int32 or tuple(src1.shape) != (n,)):
        raise ValueError(f"metric_pairs: int32 src1 [{n}] expected, got {src1.dtype} {tuple(src1.shape)}")
    if masked and (guidance is None or mean is None or mean.dtype != torch.float32 or tuple(mean.shape) != (n, 3)):
        raise ValueError(f"metric_pairs: masked pairs need the guidance and float32 mean colours [{n},3]")
    return n, k, r


def _stitch_crop_shapes(drawings, draw, offsets, r) -> Tuple[int, int, int]:
    """(n, K, D) of a ``stitch_crops`` call, or ValueError."""
    if drawings.dtype != torch.uint8 or drawings.dim() != 3 or drawings.shape[0] < 1 or drawings.shape[1] != drawings.shape[2]:
        raise ValueError(f"stitch_crops: uint8 drawings [K,D,D] expected, got {drawings.dtype} {tuple(drawings.shape)}")
    k, d = drawings.shape[0], drawings.shape[1]
    if not 1 <= int(r) <= d:
        raise ValueError(f"stitch_crops: window {r} outside 1..{d}")
    if draw.dtype != torch.int32 or draw.dim() != 1:
        raise ValueError(f"stitch_crops: int32 draw [n] expected, got {draw.dtype} {tuple(draw.shape)}")
    n = draw.shape[0]
    if offsets.dtype != torch.int32 or tuple(offsets.shape) != (n, 2):
        raise ValueError(f"stitch_crops: int32 offsets [{n},2] expected, got {offsets.dtype} {tuple(offsets.shape)}")
    return n, k, d


def _stitch_pair_shapes(fake, rects_a, rects_b, margin) -> Tuple[int, int, int]:
    """(n, R, S) of a ``stitch_pairs`` call, or ValueError."""
    if fake.dtype != torch.float32 or fake.dim() != 4 or fake.shape[1] != 3 or fake.shape[2] != fake.shape[3] or fake.shape[0] % 2:
        raise ValueError(f"stitch_pairs: float32 images [2n,3,R,R] expected, got {fake.dtype} {tuple(fake.shape)}")
    n, r = fake.shape[0] // 2, fake.shape[2]
    if int(margin) < 0 or r - 3 * int(margin) < 1:
        raise ValueError(f"stitch_pairs: margin {margin} leaves no crop window of {r} - 3 * margin pixels")
    for name, q in (("rects_a", rects_a), ("rects_b", rects_b)):
        if q.dtype != torch.int32 or tuple(q.shape) != (n, 8):
            raise ValueError(f"stitch_pairs: int32 {name} [{n},8] expected, got {q.dtype} {tuple(q.shape)}")
    return n, r, r - 3 * int(margin)


def stitch_rect(dst, src, r: int):
    """(r0, c0, r1, c1, sr0, sc0) of a composite of the ``src`` rectangle into the ``dst`` rectangle (each (rstart, cstart, rend, cend),
    ends exclusive) of r x r images, or None where ``nb_stitch_pairs_f32`` composites nothing: an empty rectangle, one that leaves the
    image, two of different extents."""
    r0, c0, r1, c1 = (int(v) for v in dst)
    sr0, sc0, sr1, sc1 = (int(v) for v in src)
    ok = 0 <= r0 < r1 <= r and 0 <= c0 < c1 <= r and sr0 >= 0 and sr1 <= r and sc0 >= 0 and sc1 <= r and sr1 - sr0 == r1 - r0 and sc1 - sc0 == c1 - c0
    return (r0, c0, r1, c1, sr0, sc0) if ok else None


def stitch_rects(crop1, crop2, margin: int) -> Tuple[np.ndarray, np.ndarray]:
    """(rects_a, rects_b), int32 [8] each: (area1, area2) of ``compute_overlaps(crop1, offset_crop(crop2))`` and of
    ``compute_overlaps(offset_crop(crop1), crop2)`` (stitching.py:248, 252), every area as (rstart, cstart, rend, cend); zeros -- "no
    composite" -- where the crops do not overlap.  Crops are (row, column, height, width)."""
    from .forger_losses import CropHelper
    out = []
    for a, b in ((crop1, CropHelper.offset_crop(crop2, margin)), (CropHelper.offset_crop(crop1, margin), crop2)):
        _, a1, a2 = CropHelper.compute_overlaps(tuple(int(v) for v in a), tuple(int(v) for v in b))
        out.append(np.zeros([8], np.int32) if a1 is None else
                   np.array([a1.rstart, a1.cstart, a1.rend, a1.cend, a2.rstart, a2.cstart, a2.rend, a2.cend], np.int32))
    return out[0], out[1]


def on_white_f32(renders: torch.Tensor) -> torch.Tensor:
    """[n,3,R,R]: ``alpha * rgb + (1 - alpha) * 1.0`` (geom_metric.py:197-198, 232-233)."""
    alpha = renders[:, 3].unsqueeze(1)
    return alpha * renders[:, :3] + (1 - alpha) * 1.0


class TileOpsBase:
    """What ``PaintingHelper`` and ``PaintSession`` call on their ``ops``, as far as it can be said without a device: the scheduling
    hooks, with defaults that do nothing (one stream, no workspaces to prepare, no noise sets, no captured graphs), and the host
    restatement of every operation that has one (drawing preparation, stroke raster, tile counts, on-white, compositing, view, the
    masked selection and the un-positioned render of the brush calibration, the evaluation masks, metric sums and composited render
    of the brush scores), on host tensors.  ``TileOps`` overrides all of them; the CPU stand-ins of the tests derive from this class and define only what has
    no restatement here (``to_device``, ``geom_tiles``, ``encode``, ``head`` / ``tail`` / ``full``, the feature-canvas operations, ``paste``)."""
    n_streams = 1
    stream_policy = 0
    graph_single = None          # None: no graphs exist; False (TileOps): they exist, off -- render_stroke switches on only the latter

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

    # -- drawing preparation and strokes: the host restatements, on host tensors (``TileOps`` runs csrc/nb_geomprep.hip, nb_strokes.hip) --
    def prepare_geometry(self, img, out_shape=None, offset=(0, 0)) -> torch.Tensor:
        """``prepare_geometry_image(img)[..., 0]`` at ``offset`` of a [out_h, out_w] uint8 buffer that is 255 elsewhere.  ``img``: decoded
        drawing, uint8 [H,W], [H,W,3] or [H,W,4], numpy or a host tensor."""
        img = img.numpy() if torch.is_tensor(img) else np.asarray(img)
        if img.dtype != np.uint8 or img.ndim not in (2, 3):
            raise ValueError(f"prepare_geometry: uint8 [H,W] or [H,W,C] expected, got {img.dtype} {tuple(img.shape)}")
        h, w = img.shape[:2]
        out = np.full((h, w) if out_shape is None else (int(out_shape[0]), int(out_shape[1])), 255, np.uint8)
        out[int(offset[0]):int(offset[0]) + h, int(offset[1]):int(offset[1]) + w] = prepare_geometry_image(img)[..., 0]
        return torch.from_numpy(out)

    def stroke_counts(self, geom: torch.Tensor, r: int, stride: int, nrows: int, ncols: int) -> torch.Tensor:
        """[nrows, ncols] int32: stroke pixels (== 0) in the r x r window of every tile."""
        return torch.from_numpy(stroke_counts_numpy(geom.numpy(), r, stride, nrows, ncols))

    def composite_on_white(self, canvas: torch.Tensor, y0: int, x0: int, h: int, w: int) -> torch.Tensor:
        """[h, w, 3] uint8: the window of the RGBA canvas at (y0, x0) over white."""
        return on_white_torch(canvas[y0:y0 + h, x0:x0 + w])

    def raster_strokes(self, strokes: StrokeList, out_shape=None, offset=(0, 0), out: Optional[torch.Tensor] = None,
                       subdiv: int = 8) -> torch.Tensor:
        """The strokes as [out_h, out_w] uint8 geometry (255 = background, 0 = stroke), drawing position (0, 0) at pixel ``offset`` =
        (off_y, off_x).  ``out`` given: the strokes are added to that geometry (every other byte untouched)."""
        if out is not None:
            raster_strokes_numpy(strokes, None, offset, subdiv, out.numpy())
            return out
        return torch.from_numpy(raster_strokes_numpy(strokes, (int(out_shape[0]), int(out_shape[1])), offset, subdiv))

    def raster_strokes_batch(self, stroke_lists, out_shape, offset=(0, 0), subdiv: int = 8) -> torch.Tensor:
        """One drawing per ``StrokeList``: [K, out_h, out_w] uint8 geometry, each as ``raster_strokes`` gives it for that list alone."""
        shape = (int(out_shape[0]), int(out_shape[1]))
        if not len(stroke_lists):
            raise ValueError("raster_strokes_batch: no stroke lists")
        return torch.from_numpy(np.stack([raster_strokes_numpy(s, shape, offset, subdiv) for s in stroke_lists]))

    # -- brush calibration: the torch restatements (``TileOps`` runs csrc/nb_select.hip and the HIP generator) --
    def masked_kth_largest(self, x: torch.Tensor, mask: torch.Tensor, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """(kth [n] float32, n_masked [n] int32): per image of ``x`` [n,1,h,w] or [n,h,w] (a strided view is fine) the ``k``-th largest
        of the values that ``mask`` [m, ...] (bool or uint8; image i takes mask i % m) includes, in the order of
        ``torch.topk(largest=True)``: NaN above +inf.  NaN where fewer than ``k`` values are included."""
        n, count, m = _select_shapes(x, mask, k)
        flat, inc = x.reshape(n, count), mask.reshape(m, count) != 0
        kth = torch.full([n], float("nan"), dtype=torch.float32, device=x.device)
        n_masked = torch.zeros([n], dtype=torch.int32, device=x.device)
        for i in range(n):
            v = flat[i][inc[i % m]]
            n_masked[i] = v.numel()
            if v.numel() >= k:
                kth[i] = torch.topk(v, k)[0][k - 1]
        return kth, n_masked

    def triad_debug(self, ws: torch.Tensor, geom_feats):
        """(img [n,3,R,R], debug data with ``uvs`` [n,3,R,R] and ``colors`` [n,3,3]) of an un-positioned render with the checkpoint's
        constant noise and without brush noise buffers: what StyleUVSMapper renders (mapper.py:80-92).  This restatement renders
        sample by sample: torch picks its matrix routines by batch size, and a sample's result must not depend on what else is in the
        batch (the batched catalogue is held to the one-brush calls bit for bit on this route)."""
        syn = getattr(self.G.synthesis, "forward", self.G.synthesis)
        takes = any(p.name == "noise_mode" or p.kind is p.VAR_KEYWORD for p in inspect.signature(syn).parameters.values())
        kw = {"noise_mode": "const"} if takes else {}
        feats = list(geom_feats)
        outs = [self.G.forward_pre_mapped(ws[i:i + 1], [f[i:i + 1] for f in feats], return_debug_data=True, **kw) for i in range(ws.shape[0])]
        dbg = {k: torch.cat([d[k] for _, d in outs]) for k in ("uvs", "colors")}
        return torch.cat([img for img, _ in outs]), dbg

    # -- brush scores: the torch restatements (``TileOps`` runs csrc/nb_metrics.hip and the HIP generator) --
    def eval_masks(self, geom: torch.Tensor) -> EvalMasks:
        """The evaluation masks of the drawings ``geom`` [K,R,R] float32 (0 = stroke): the Gaussian applied twice
        (geom_metric.py:153) and the two masks of ``compute_transparency_metrics``, with their counts."""
        if geom.dtype != torch.float32 or geom.dim() != 3 or geom.shape[1] != geom.shape[2]:
            raise ValueError(f"eval_masks: float32 drawings [K,R,R] expected, got {geom.dtype} {tuple(geom.shape)}")
        geom = geom.contiguous()
        blur = gaussian_blur_torch(gaussian_blur_torch(geom.unsqueeze(1))).squeeze(1)
        bg, fg = blur > BG_THRESH, geom < FG_THRESH
        k = geom.shape[0]
        return EvalMasks(geom, blur, bg.to(torch.uint8) | (fg.to(torch.uint8) << 1), bg.reshape(k, -1).sum(dim=1).to(torch.int32),
                         fg.reshape(k, -1).sum(dim=1).to(torch.int32))

    def brush_metrics(self, renders: torch.Tensor, target_rgb: torch.Tensor, masks: EvalMasks, lab_thresh: float = 10,
                      ignore_transparency: bool = False, want_deltas: bool = False):
        """(sums [n,4] float32, alpha [n, R*R] float32[, deltas [n,R,R]]) of ``renders`` [n,4,R,R] in 0..1 (a view is fine) against
        ``target_rgb`` [n,3]; image i lies on drawing i % K of ``masks``.  With dE the Lab distance of a pixel to the target
        (color_metric.py:29-49) and the float weight w = 1 - geom: sums = (sum w dE, sum w [dE > lab_thresh], sum w, sum of alpha over
        the background pixels); ``alpha`` is every render's alpha plane, dense."""
        n, k, r = _metric_shapes(renders, target_rgb, masks)
        deltas = lab_deltas_torch(target_rgb, renders, ignore_transparency)
        idx = torch.arange(n, device=renders.device) % k
        w = (1 - masks.geom)[idx]
        alpha = renders[:, 3]
        bg = (masks.mask[idx] & 1).to(torch.float32)
        sums = torch.stack([torch.sum(w * deltas, dim=(1, 2)), torch.sum((deltas > lab_thresh).to(torch.float32) * w, dim=(1, 2)),
                            torch.sum(w, dim=(1, 2)), torch.sum(alpha * bg, dim=(1, 2))], dim=1)
        out = (sums, alpha.reshape(n, r * r).contiguous())
        return out + (deltas,) if want_deltas else out

    # -- inputs of the perceptual brush scores: the torch restatements (``TileOps`` runs csrc/nb_metric_patches.hip) --
    def bg_guidance(self, geom: torch.Tensor) -> BgGuidance:
        """The guidance of the background metrics for the drawings ``geom`` [K,R,R] float32 (0 = stroke): the Gaussian applied ONCE
        (geom_metric.py:235) and the number of pixels above 0.99 (geom_metric.py:238-239)."""
        if geom.dtype != torch.float32 or geom.dim() != 3 or geom.shape[1] != geom.shape[2]:
            raise ValueError(f"bg_guidance: float32 drawings [K,R,R] expected, got {geom.dtype} {tuple(geom.shape)}")
        geom = geom.contiguous()
        blur1 = gaussian_blur_torch(geom.unsqueeze(1)).squeeze(1)
        return BgGuidance(geom, blur1, (blur1 > BG_THRESH_PATCHES).reshape(geom.shape[0], -1).sum(dim=1).to(torch.int32))

    def bg_mean_colors(self, renders: torch.Tensor, guidance: BgGuidance) -> torch.Tensor:
        """[n,3] float32: the mean on-white colour of every render [n,4,R,R] over its drawing's background, image i on drawing i % K
        (geom_metric.py:232-241); zeros where a drawing has no background."""
        n, k, _ = _render_shapes("bg_mean_colors", renders, guidance)
        rgb = on_white_f32(renders)
        bg_mask = (guidance.blur1[torch.arange(n, device=renders.device) % k].unsqueeze(1) > BG_THRESH_PATCHES).to(torch.float32)
        return torch.sum(rgb * bg_mask, dim=(2, 3)) / torch.clamp(torch.sum(bg_mask, dim=(2, 3)), min=1.0)

    def metric_pairs(self, renders: torch.Tensor, guidance: Optional[BgGuidance], mean: Optional[torch.Tensor], off0: torch.Tensor,
                     off1: torch.Tensor, src1: Optional[torch.Tensor], p: int, transpose: bool = True, masked: bool = True) -> torch.Tensor:
        """[2n,3,p,p] float32 in -1..1, the LPIPS input of n pairs: rows :n the ``p`` x ``p`` window of image i at ``off0[i]`` = (row,
        column), rows n: the window of image ``src1[i]`` (None: i) at ``off1[i]``, transposed with ``transpose``; with ``masked``
        every pixel that is not background (blurred guidance above 0.99) in BOTH patches takes ``mean[i]`` in both
        (geom_metric.py:244-259).  Unmasked, with ``p`` = R and zero offsets: the pairs of ``compute_lpips_across_geo``."""
        n, k, r = _pair_shapes(renders, guidance, mean, off0, off1, src1, p, masked)
        p = int(p)
        rgb = on_white_f32(renders)
        idx = torch.arange(n, device=renders.device)
        if masked:
            rgb = torch.cat([rgb, guidance.blur1[idx % k].unsqueeze(1)], dim=1)
        o0, o1 = off0.clamp(0, r - p).tolist(), off1.clamp(0, r - p).tolist()
        src = idx.tolist() if src1 is None else src1.clamp(0, n - 1).tolist()
        patches0 = torch.stack([rgb[i, :, o0[i][0]:o0[i][0] + p, o0[i][1]:o0[i][1] + p] for i in range(n)]) if n else rgb[:, :, :p, :p]
        patches1 = torch.stack([rgb[j, :, o1[i][0]:o1[i][0] + p, o1[i][1]:o1[i][1] + p] for i, j in enumerate(src)]) if n else rgb[:, :, :p, :p]
        if transpose:
            patches1 = patches1.permute(0, 1, 3, 2)
        if masked:
            bg_mask = torch.logical_and(patches0[:, 3] > BG_THRESH_PATCHES, patches1[:, 3] > BG_THRESH_PATCHES).to(torch.float32).unsqueeze(1)
            mc = mean.unsqueeze(-1).unsqueeze(-1)
            patches0 = bg_mask * patches0[:, :3] + (1 - bg_mask) * mc
            patches1 = bg_mask * patches1[:, :3] + (1 - bg_mask) * mc
        return torch.cat([patches0 * 2 - 1.0, patches1 * 2 - 1.0]).contiguous()

    # -- inputs of the stitching scores: the torch restatements (``TileOps`` runs csrc/nb_stitch_metrics.hip and the HIP generator) --
    def stitch_crops(self, drawings: torch.Tensor, draw: torch.Tensor, offsets: torch.Tensor, r: Optional[int] = None) -> torch.Tensor:
        """[n,1,R,R] float32, the generator's geometry input of n windows of full-size drawings: window i is the R x R window of
        ``drawings[draw[i]]`` ([K,D,D] uint8, 0 = stroke) at ``offsets[i]`` = (row, column), value / 255 (metric_main.py:183-189).
        ``r``: the window's side (the engine's patch width).  An index is clamped into 0..K - 1 and an offset into 0..D - R."""
        r = int(self.patch_width if r is None else r)
        n, k, d = _stitch_crop_shapes(drawings, draw, offsets, r)
        # value / 255 through a host-computed table: device division is not correctly rounded
        lut = torch.from_numpy(np.arange(256, dtype=np.float32) / np.float32(255)).to(drawings.device)
        j, o = draw.clamp(0, k - 1).tolist(), offsets.clamp(0, d - r).tolist()
        if not n:
            return torch.zeros([0, 1, r, r], dtype=torch.float32, device=drawings.device)
        return torch.stack([lut[drawings[j[i], o[i][0]:o[i][0] + r, o[i][1]:o[i][1] + r].to(torch.int64)] for i in range(n)]).unsqueeze(1).contiguous()

    def stitch_pairs(self, fake: torch.Tensor, rects_a: torch.Tensor, rects_b: torch.Tensor, margin: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """(x [4n,3,S,S], l1 [2n]) of the raw generator images ``fake`` [2n,3,R,R] (rows :n the first crops, rows n: the second) of
        ``RandomStitcher.generate_with_stitching``: the LPIPS input of the 2n pairs of ``compute_stitching_metrics``
        (geom_metric.py:165-187) in the row convention of ``metric_pairs`` -- rows :n crop(fake1), n:2n crop(fake2), 2n:3n
        crop(fake1 with fake2's pixels), 3n: crop(fake2 with fake1's pixels) -- and the sum of |first - second| of every pair.
        ``rects_a`` / ``rects_b`` [n,8] int32: per sample the two areas (``stitch_rects``) of the first and of the second composite;
        a pair that ``stitch_rect`` refuses composites nothing.  crop(img) = img[:, :, margin:R - 2 margin, margin:R - 2 margin]: the
        reference's asymmetric crop, S = R - 3 margin.  Nothing is rescaled: every value of x is a copy of a value of ``fake``."""
        n, r, s = _stitch_pair_shapes(fake, rects_a, rects_b, margin)
        m = int(margin)
        f1, f2 = fake[:n], fake[n:]
        c1, c2 = f1.clone(), f2.clone()
        for i, (qa, qb) in enumerate(zip(rects_a.tolist(), rects_b.tolist())):
            a, b = stitch_rect(qa[:4], qa[4:], r), stitch_rect(qb[4:], qb[:4], r)
            if a is not None:                                              # CropHelper.composite(fake1, fake2, area1, area2)
                c1[i, :, a[0]:a[2], a[1]:a[3]] = f2[i, :, a[4]:a[4] + a[2] - a[0], a[5]:a[5] + a[3] - a[1]]
            if b is not None:                                              # CropHelper.composite(fake2, fake1, area2, area1)
                c2[i, :, b[0]:b[2], b[1]:b[3]] = f1[i, :, b[4]:b[4] + b[2] - b[0], b[5]:b[5] + b[3] - b[1]]
        x = torch.cat([t[:, :, m:r - 2 * m, m:r - 2 * m] for t in (f1, f2, c1, c2)]).contiguous()
        return x, (x[:2 * n] - x[2 * n:]).abs().sum(dim=(1, 2, 3))

    def render_img(self, ws: torch.Tensor, geom_feats, positions: torch.Tensor, noise_set=None) -> torch.Tensor:
        """[n,3,R,R] float32: the generator's raw image with the noise read at ``positions`` [n,2] and the checkpoint's constant noise
        -- no compositing, no sfactor, what ``RandomStitcher.generate_with_stitching`` scores (stitching.py:244-245)."""
        if noise_set is not None:
            raise ValueError("render_img: this ops has no noise sets")
        syn = getattr(self.G.synthesis, "forward", self.G.synthesis)
        takes = any(p.name == "noise_mode" or p.kind is p.VAR_KEYWORD for p in inspect.signature(syn).parameters.values())
        return self.G.forward_pre_mapped(ws, geom_feats, positions=positions, **({"noise_mode": "const"} if takes else {}))

    def render_rgba(self, ws: torch.Tensor, geom_feats, user_colors=None, sfactor=None, noise_set=None) -> torch.Tensor:
        """[n,4,R,R] float32 in 0..1: the un-positioned "clear" render of the paint engine (brush.py:763-792) with the checkpoint's
        constant noise; ``user_colors`` [n,3,3] replace the generator's colours where they are not NaN, ``sfactor`` [n] stretches the
        background weight (mapper.py:52-72).  This restatement composites ``triad_debug``'s weights and colours in torch."""
        if noise_set is not None:
            raise ValueError("render_rgba: this ops has no noise sets")
        _, dbg = self.triad_debug(ws, geom_feats)
        uvs, colors = dbg["uvs"], (dbg["colors"] + 1) / 2.0
        if sfactor is not None:
            sp = torch.clamp(torch.as_tensor(sfactor, dtype=uvs.dtype).reshape(-1, 1, 1, 1) * uvs[:, 2:3], max=1.0)
            f = torch.where(1 - sp <= 0.000001, torch.zeros_like(sp), (1 - sp) / (uvs[:, 0:1] + uvs[:, 1:2]))
            uvs = torch.cat([f * uvs[:, 0:1], f * uvs[:, 1:2], sp], dim=1)
        if user_colors is not None:
            colors = torch.where(torch.isnan(user_colors), colors, user_colors.to(colors.dtype))
        stroke = torch.sum(uvs.unsqueeze(1) * colors.unsqueeze(-1).unsqueeze(-1), dim=2)
        return torch.cat([stroke, torch.sum(uvs[:, 0:2], dim=1, keepdim=True)], dim=1)

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
            ws = ws.to(self.device, torch.float32)
            if ws.dim() == 3 and ws.shape[1] == 1 and self.cfg.num_ws > 1:     # a brush projected into W, not W+ (project_main.py:460)
                ws = ws.expand(ws.shape[0], self.cfg.num_ws, ws.shape[2]).contiguous()
            return ws
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
        return self.triad_debug(ws, geom_feats)[1]["uvs"][:, 2:3]

    def triad_debug(self, ws: torch.Tensor, geom_feats):
        """(img, debug data with ``uvs`` and ``colors``) of ONE un-positioned generator pass over the batch, constant noise."""
        return self.G.forward_pre_mapped(ws, geom_feats, return_debug_data=True, noise_mode="const")

    # -- masked selection (csrc/nb_select.hip) --
    def masked_kth_largest(self, x: torch.Tensor, mask: torch.Tensor, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """(kth [n] float32, n_masked [n] int32) on the device, one launch (``nb_masked_kth_largest_f32``): per image of ``x``
        [n,1,h,w] or [n,h,w] the ``k``-th largest of the values that ``mask`` [m, ...] (bool or uint8; image i takes mask i % m)
        includes, NaN above +inf; NaN where fewer than ``k`` are included.  A view whose images are dense (``uvs[:, 2]``) is read in place."""
        n, count, m = _select_shapes(x, mask, k)
        if x.device != self.device or mask.device != self.device:
            raise ValueError("masked_kth_largest: x and mask must be on the engine's device")
        w = x.shape[-1]
        if x.stride(-1) != 1 or x.stride(-2) != w or (n > 1 and x.stride(0) < count):
            x = x.contiguous()
        mask = mask.contiguous()
        mask = mask.view(torch.uint8) if mask.dtype == torch.bool else mask
        kth = torch.empty([n], dtype=torch.float32, device=self.device)
        n_masked = torch.empty([n], dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().nb_masked_kth_largest_f32(_p(x), max(int(x.stride(0)), count), _p(mask), m, count, int(k), n, _p(kth),
                                                            _p(n_masked), self._stream()), "masked_kth_largest")
        return kth, n_masked

    # -- brush scores (csrc/nb_metrics.hip) --
    def eval_masks(self, geom: torch.Tensor) -> EvalMasks:
        """The evaluation masks of the drawings ``geom`` [K,R,R] float32 on the device, one launch (``nb_eval_masks_f32``)."""
        if geom.dtype != torch.float32 or geom.dim() != 3 or geom.shape[1] != geom.shape[2] or geom.device != self.device:
            raise ValueError(f"eval_masks: float32 drawings [K,R,R] on the engine's device expected, got {geom.dtype} {tuple(geom.shape)}")
        geom = geom.contiguous()
        k, r = geom.shape[0], geom.shape[1]
        blur, mask = torch.empty_like(geom), torch.empty([k, r, r], dtype=torch.uint8, device=self.device)
        n_bg, n_fg = (torch.empty([k], dtype=torch.int32, device=self.device) for _ in range(2))
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().nb_eval_masks_f32(_p(geom), k, r, _p(blur), _p(mask), _p(n_bg), _p(n_fg), self._stream()), "eval_masks")
        return EvalMasks(geom, blur, mask, n_bg, n_fg)

    def brush_metrics(self, renders: torch.Tensor, target_rgb: torch.Tensor, masks: EvalMasks, lab_thresh: float = 10,
                      ignore_transparency: bool = False, want_deltas: bool = False):
        """(sums [n,4], alpha [n, R*R][, deltas [n,R,R]]) on the device (``nb_brush_metrics_f32``: one pass over the renders and a
        fixed-order finish; the same input gives the same bits).  A view whose samples are dense [4,R,R] blocks is read in place."""
        n, k, r = _metric_shapes(renders, target_rgb, masks)
        if renders.device != self.device or target_rgb.device != self.device or masks.geom.device != self.device:
            raise ValueError("brush_metrics: renders, colours and masks must be on the engine's device")
        count = r * r
        if renders.stride(3) != 1 or renders.stride(2) != r or renders.stride(1) != count or (n > 1 and renders.stride(0) < 4 * count):
            renders = renders.contiguous()
        target_rgb = target_rgb.contiguous()
        sums = torch.empty([n, 4], dtype=torch.float32, device=self.device)
        alpha = torch.empty([n, count], dtype=torch.float32, device=self.device)
        deltas = torch.empty([n, r, r], dtype=torch.float32, device=self.device) if want_deltas else None
        partials = torch.empty([n, _lib.NB_BRUSH_METRICS_PARTS, 4], dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().nb_brush_metrics_f32(_p(renders), max(int(renders.stride(0)), 4 * count), _p(target_rgb), _p(masks.geom),
                                                       _p(masks.mask), k, r, n, float(lab_thresh), int(bool(ignore_transparency)), _p(sums),
                                                       _p(alpha), _p(deltas), _p(partials), self._stream()), "brush_metrics")
        return (sums, alpha, deltas) if want_deltas else (sums, alpha)

    # -- inputs of the perceptual brush scores (csrc/nb_metric_patches.hip) --
    def _dense_renders(self, renders: torch.Tensor, r: int) -> torch.Tensor:
        """``renders`` as it is where its samples are dense [4,R,R] blocks (a view is read in place), else a dense copy."""
        count, n = r * r, renders.shape[0]
        if renders.stride(3) != 1 or renders.stride(2) != r or renders.stride(1) != count or (n > 1 and renders.stride(0) < 4 * count):
            return renders.contiguous()
        return renders

    def bg_guidance(self, geom: torch.Tensor) -> BgGuidance:
        """The once-blurred guidance of the drawings ``geom`` [K,R,R] float32 and its background counts, one launch
        (``nb_bg_guidance_f32``)."""
        if geom.dtype != torch.float32 or geom.dim() != 3 or geom.shape[1] != geom.shape[2] or geom.device != self.device:
            raise ValueError(f"bg_guidance: float32 drawings [K,R,R] on the engine's device expected, got {geom.dtype} {tuple(geom.shape)}")
        geom = geom.contiguous()
        k, r = geom.shape[0], geom.shape[1]
        blur1, n_bg = torch.empty_like(geom), torch.empty([k], dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().nb_bg_guidance_f32(_p(geom), k, r, _p(blur1), _p(n_bg), self._stream()), "bg_guidance")
        return BgGuidance(geom, blur1, n_bg)

    def bg_mean_colors(self, renders: torch.Tensor, guidance: BgGuidance) -> torch.Tensor:
        """[n,3] on the device (``nb_bg_mean_colors_f32``: one pass over the renders and a fixed-order finish)."""
        n, k, r = _render_shapes("bg_mean_colors", renders, guidance)
        if renders.device != self.device or guidance.blur1.device != self.device:
            raise ValueError("bg_mean_colors: renders and guidance must be on the engine's device")
        renders = self._dense_renders(renders, r)
        mean = torch.empty([n, 3], dtype=torch.float32, device=self.device)
        partials = torch.empty([n, _lib.NB_BG_MEAN_PARTS, 3], dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().nb_bg_mean_colors_f32(_p(renders), max(int(renders.stride(0)), 4 * r * r), _p(guidance.blur1.contiguous()),
                                                        _p(guidance.n_bg), k, r, n, _p(partials), _p(mean), self._stream()), "bg_mean_colors")
        return mean

    def metric_pairs(self, renders: torch.Tensor, guidance: Optional[BgGuidance], mean: Optional[torch.Tensor], off0: torch.Tensor,
                     off1: torch.Tensor, src1: Optional[torch.Tensor], p: int, transpose: bool = True, masked: bool = True) -> torch.Tensor:
        """[2n,3,p,p] on the device, one launch (``nb_metric_pairs_f32``): both sides of every pair in one buffer."""
        n, k, r = _pair_shapes(renders, guidance, mean, off0, off1, src1, p, masked)
        tensors = [renders, off0, off1] + ([src1] if src1 is not None else []) + ([guidance.blur1, mean] if masked else [])
        if any(t.device != self.device for t in tensors):
            raise ValueError("metric_pairs: renders, guidance, colours and the plan must be on the engine's device")
        renders = self._dense_renders(renders, r)
        out = torch.empty([2 * n, 3, int(p), int(p)], dtype=torch.float32, device=self.device)
        flags = (_lib.NB_METRIC_PAIRS_TRANSPOSE if transpose else 0) | (_lib.NB_METRIC_PAIRS_MASKED if masked else 0)
        blur1 = guidance.blur1.contiguous() if masked else None
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().nb_metric_pairs_f32(_p(renders), max(int(renders.stride(0)), 4 * r * r), _p(blur1),
                                                      _p(mean.contiguous()) if masked else None, _p(off0.contiguous()), _p(off1.contiguous()),
                                                      None if src1 is None else _p(src1.contiguous()), k, r, int(p), n, flags, _p(out),
                                                      self._stream()), "metric_pairs")
        return out

    # -- inputs of the stitching scores (csrc/nb_stitch_metrics.hip) --
    def stitch_crops(self, drawings: torch.Tensor, draw: torch.Tensor, offsets: torch.Tensor, r: Optional[int] = None) -> torch.Tensor:
        """[n,1,R,R] on the device, one launch (``nb_stitch_crops_u8``): n windows of the full-size drawings as geometry input."""
        r = int(self.patch_width if r is None else r)
        n, k, d = _stitch_crop_shapes(drawings, draw, offsets, r)
        if any(t.device != self.device for t in (drawings, draw, offsets)):
            raise ValueError("stitch_crops: drawings and windows must be on the engine's device")
        out = torch.empty([n, 1, r, r], dtype=torch.float32, device=self.device)
        if n == 0:                                                         # (empty tensors have no address to hand over)
            return out
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().nb_stitch_crops_u8(_p(drawings.contiguous()), k, d, _p(draw.contiguous()), _p(offsets.contiguous()), n, r, _p(out),
                                                     self._stream()), "stitch_crops")
        return out

    def stitch_pairs(self, fake: torch.Tensor, rects_a: torch.Tensor, rects_b: torch.Tensor, margin: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """(x [4n,3,S,S], l1 [2n]) on the device (``nb_stitch_pairs_f32``: one pass over the images and a fixed-order finish; the same
        input gives the same bits).  A view whose images are dense [3,R,R] blocks is read in place."""
        n, r, s = _stitch_pair_shapes(fake, rects_a, rects_b, margin)
        if any(t.device != self.device for t in (fake, rects_a, rects_b)):
            raise ValueError("stitch_pairs: images and rectangles must be on the engine's device")
        count = r * r
        if fake.stride(3) != 1 or fake.stride(2) != r or fake.stride(1) != count or (2 * n > 1 and fake.stride(0) < 3 * count):
            fake = fake.contiguous()
        x = torch.empty([4 * n, 3, s, s], dtype=torch.float32, device=self.device)
        l1 = torch.empty([2 * n], dtype=torch.float32, device=self.device)
        if n == 0:
            return x, l1
        partials = torch.empty([n, _lib.NB_STITCH_PARTS, 2], dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().nb_stitch_pairs_f32(_p(fake), max(int(fake.stride(0)), 3 * count), _p(rects_a.contiguous()), _p(rects_b.contiguous()),
                                                      n, r, int(margin), _p(x), _p(l1), _p(partials), self._stream()), "stitch_pairs")
        return x, l1

    def render_img(self, ws: torch.Tensor, geom_feats, positions: torch.Tensor, noise_set=None) -> torch.Tensor:
        """[n,3,R,R] float32: ONE positioned generator pass with the checkpoint's constant noise, the raw image."""
        kw = {} if noise_set is None else {"noise_set": noise_set}
        return self.G.forward_pre_mapped(ws, geom_feats, positions=positions, noise_mode="const", **kw)

    def render_rgba(self, ws: torch.Tensor, geom_feats, user_colors=None, sfactor=None, noise_set=None) -> torch.Tensor:
        """[n,4,R,R] float32 in 0..1: ONE un-positioned "clear" generator pass, composited in the ToRGB launch."""
        kw = {} if noise_set is None else {"noise_set": noise_set}
        _, rgba, _ = self.G.render_triad(ws=ws, geom_feature=geom_feats, want_u8=False, want_f32=True, render_mode="clear", positions=None,
                                         user_colors=user_colors, sfactor=sfactor, **kw)
        return rgba

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
                cells = cell_box(box, hc, wc)
                if cells is None:
                    return mask
                mask_out = mask.clone()
                _lib.check(_lib.lib().nb_canvas_replay_box_f32(_p(tiles), t, c, hw, _p(tile_yx), _p(alpha0), crop, _p(canvas),
                                                               _p(mask), _p(mask_out), hc, wc, _p(cell_off), _p(cell_tiles),
                                                               *cells, self._stream()), "canvas_replay")
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
        hc, wc = mask.shape
        c = pieces[0][0].shape[0]
        arr = (_lib.NbTilePiece * len(pieces))()
        for i, (v, cy, cx, ly0, lx0) in enumerate(pieces):
            assert v.dtype == torch.float32 and v.stride(2) == 1 and v.shape[0] == c
            arr[i] = _lib.NbTilePiece(v.data_ptr(), v.stride(0), v.stride(1), cy, cx, v.shape[1], v.shape[2], ly0, lx0)
        table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(self.device, non_blocking=True)
        cells = cell_box(box, hc, wc)
        if cells is None:
            return mask
        mask_out = mask.clone()
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().nb_canvas_replay_pieces_f32(_p(table), len(pieces), c, hw, _p(alpha0), crop, _p(canvas),
                                                              _p(mask), _p(mask_out), hc, wc, _p(cell_off), _p(cell_pieces),
                                                              *cells, self._stream()), "canvas_replay_pieces")
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

    def raster_strokes_batch(self, stroke_lists, out_shape, offset=(0, 0), subdiv: int = 8) -> torch.Tensor:
        """One drawing per ``StrokeList``: [K, out_h, out_w] uint8 on the device, byte for byte what ``raster_strokes`` gives for each
        list alone, from one ``nb_spline_flatten_f32`` launch over all splines and one ``nb_raster_batch_u8`` launch over all
        drawings.  Polyline rows are uploaded and joined with their drawing's spline rows on the device; nothing is read back."""
        from .drawings import raster_batch
        k = len(stroke_lists)
        if not k:
            raise ValueError("raster_strokes_batch: no stroke lists")
        merged = StrokeList()
        for s in stroke_lists:
            merged._ctrl.extend(s._ctrl)
        spl = self.stroke_segments(merged, subdiv)                  # all splines, drawing after drawing
        n_spl = np.array([s.spline_segment_count(subdiv) for s in stroke_lists], np.int64)
        polys = [s.polyline_segments() for s in stroke_lists]
        if any(p.shape[0] for p in polys):
            ends = np.cumsum(n_spl)
            pieces = []
            for i, p in enumerate(polys):
                pieces += [self.to_device(p), spl[int(ends[i] - n_spl[i]):int(ends[i])]]
            segs = torch.cat(pieces)
        else:
            segs = spl
        seg_off = np.zeros(k + 1, np.int32)
        np.cumsum(n_spl + np.array([p.shape[0] for p in polys], np.int64), out=seg_off[1:])
        return raster_batch(segs, seg_off, out_shape, offset, device=self.device)
