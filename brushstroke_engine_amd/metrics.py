"""Brush scores: the numbers the reference reports per brush (``paint_engine_metric_loop``, forger/metrics/metric_main.py:105-236),
computed where the renders are.

    LAB_E%, LAB_L2                       how well the stroke takes the user's primary colour, in CIE Lab
                                         (``compute_lab_metrics``, forger/metrics/color_metric.py:29-70)
    BG_CLARITY_MEAN, FG_OPACITY_MEDIAN   how clear the background and how opaque the stroke is
                                         (``compute_transparency_metrics``, forger/metrics/geom_metric.py:126-162)

The three functions keep the reference's signatures and keys, so a caller of the reference can switch; ``BrushEvaluator`` scores a
whole library in batches: ``floor(batch / K)`` brushes share a generator pass on the K drawings, ``ops.brush_metrics`` reduces the
pass's renders to four sums per image in one launch, and the pooled median is ``ops.masked_kth_largest`` on the alpha planes it
leaves.  Nothing is copied to the host until the ``BrushScores`` are assembled.

With an LPIPS network (``perceptual.LPIPS``; the reference uses ``alex``) three perceptual numbers join them:

    LPIPS_UNIFORM_BG_multicolor          whether the background is uniform: LPIPS between two random windows of a render (the second
    LPIPS_UNIFORM_BG                     transposed) with everything but the common background filled with the background's mean colour
                                         (``compute_uniform_bg_lpips_metric``, forger/metrics/geom_metric.py:207-262) -- on the render with
                                         random primary colours, and on a second render with the brush's own colours, pairs permuted
    LPIPS_ACROSS_GEO                     whether the brush looks the same on different drawings: LPIPS between the K own-colour
                                         renders and a permutation of them (``compute_lpips_across_geo``, geom_metric.py:190-204)

``ops.bg_mean_colors`` and ``ops.metric_pairs`` (csrc/nb_metric_patches.hip) write the network's input of both sides of all pairs of
a pass into one buffer, and ``LPIPS.pair_distance`` runs the trunk once over it.  The random windows and permutations come from a
seeded plan (``default_crops``): the reference draws them from the process-global stream, so no seed reproduces ITS draws; the
distribution is the same.

With full-size drawings (``StitchSetup``) the last two columns of the reference's files join them:

    STITCH_LPIPS, STITCH_L1              how well the brush survives being painted tile by tile: two positioned raw renders of
                                         overlapping crops of a full-size drawing, each with the other's pixels composited into
                                         the overlap, against themselves (metric_main.py:181-200, ``RandomStitcher.generate_with_stitching``,
                                         ``compute_stitching_metrics``, geom_metric.py:165-187)

``ops.stitch_crops`` gathers the crops of a pass, ``ops.render_img`` renders both sides in one generator pass, and
``ops.stitch_pairs`` (csrc/nb_stitch_metrics.hip) writes the four cropped images of every sample into one LPIPS input and sums the
absolute differences in the same launch; the crops and noise positions come from ``default_stitch_plan``.  ``BG_LPIPS*`` is not
part of this module.
"""
from __future__ import annotations

import dataclasses
import inspect
import json
import os
from typing import Callable, Dict, List, Optional, Sequence

import numpy as np
import torch

from .tile_ops import EvalMasks, TileOpsBase, lab_deltas_torch, stitch_rects

KEYS = ("BG_CLARITY_MEAN", "FG_OPACITY_MEDIAN", "LAB_E%", "LAB_L2")          # sorted, the column order of the reference's files
PERCEPTUAL_KEYS = ("LPIPS_ACROSS_GEO", "LPIPS_UNIFORM_BG", "LPIPS_UNIFORM_BG_multicolor")          # sorted likewise; they sort behind KEYS
STITCH_KEYS = ("STITCH_L1", "STITCH_LPIPS")                                  # sorted likewise; they sort behind PERCEPTUAL_KEYS
_HIGHER_IS_BETTER = {"BG_CLARITY_MEAN": True, "FG_OPACITY_MEDIAN": True, "LAB_E%": False, "LAB_L2": False, "LPIPS_ACROSS_GEO": False,
                     "LPIPS_UNIFORM_BG": False, "LPIPS_UNIFORM_BG_multicolor": False, "STITCH_L1": False, "STITCH_LPIPS": False}


def _fg_pool(masks: EvalMasks):
    """(the foreground bits of all K drawings as ONE mask [1, K*R*R] uint8, their number N): what the pooled median selects on.
    Reading N waits for the device once per set of drawings."""
    return ((masks.mask >> 1) & 1).reshape(1, -1).contiguous(), int(masks.n_fg.sum())


def pooled_scores(ops, sums: torch.Tensor, alpha: torch.Tensor, masks: EvalMasks, fg_mask: torch.Tensor, n_fg: int) -> torch.Tensor:
    """[nb, 4] in the order of ``KEYS``, where ``sums`` is: the scores of nb brushes from the sums [nb*K,4] and alpha planes [nb*K,R*R]
    of ``ops.brush_metrics``, brush-major.  LAB_* are means over a brush's K images of the per-image values; the clarity and the
    median pool the K images (the reference hands all K renders of a brush to ``compute_transparency_metrics`` at once).  The median is
    ``torch.median``'s LOWER median: the k-th largest of the N foreground alphas with k = N - (N - 1) // 2."""
    k, count = masks.geom.shape[0], alpha.shape[1]
    nb = sums.shape[0] // k
    lab_e = (sums[:, 1] / sums[:, 2].clip(min=1) * 100).view(nb, k).mean(dim=1)
    lab_l2 = (sums[:, 0] / count).view(nb, k).mean(dim=1)
    clarity = 1 - sums[:, 3].view(nb, k).sum(dim=1) / masks.n_bg.sum().to(torch.float32)          # 0 / 0 = NaN: no background at all
    if n_fg >= 1:
        median, _ = ops.masked_kth_largest(alpha.view(nb, 1, k * count), fg_mask, n_fg - (n_fg - 1) // 2)
    else:
        median = torch.full([nb], float("nan"), dtype=torch.float32, device=sums.device)
    return torch.stack([clarity, median, lab_e, lab_l2], dim=1)


# ---------------------------------------------------------------------------------------------------------------------
# the reference's three functions
# ---------------------------------------------------------------------------------------------------------------------
def compute_lab_deltas(target_colors, renders, ignore_transparency=False):
    """[B,W,W]: Lab distance between every pixel of ``renders`` [B,4,W,W] (0..1; over white unless ``ignore_transparency``) and the
    image's colour ``target_colors`` [B,3] (color_metric.py:29-49), in torch where the tensors are."""
    return lab_deltas_torch(target_colors, renders, ignore_transparency)


def _masks_for(ops, geom):
    ops = TileOpsBase() if ops is None else ops
    return ops, ops.eval_masks(geom.squeeze(1).to(torch.float32).contiguous())


def compute_lab_metrics(target_colors, renders, geom, lab_thresh=10, ignore_transparency=False, ops=None):
    """{'LAB_E%', 'LAB_L2'} of ``renders`` [B,4,W,W] on the guidance ``geom`` [B,1,W,W] (0 = stroke), every image with its own
    colour and drawing, averaged over the batch (color_metric.py:52-70).  ``ops``: whose ``brush_metrics`` computes the sums
    (``TileOps``: one launch); None: the torch restatement where the tensors are."""
    ops, masks = _masks_for(ops, geom)
    sums, _ = ops.brush_metrics(renders, target_colors, masks, lab_thresh, ignore_transparency)
    count = renders.shape[2] * renders.shape[3]
    return {"LAB_E%": torch.mean(sums[:, 1] / sums[:, 2].clip(min=1) * 100).item(), "LAB_L2": torch.mean(sums[:, 0] / count).item()}


def compute_transparency_metrics(renders, geom, ops=None):
    """{'BG_CLARITY_MEAN', 'FG_OPACITY_MEDIAN'} of the renders [B,4,W,W] of ONE brush on ``geom`` [B,1,W,W], all images pooled
    (geom_metric.py:143-162): one minus the mean alpha where the guidance blurred twice exceeds 0.999, and the lower median of alpha
    where the guidance lies below 0.3.  A batch without such pixels gives NaN for that value (the reference returns NaN for the mean
    and raises in ``torch.median`` on an empty selection)."""
    ops, masks = _masks_for(ops, geom)
    fg_mask, n_fg = _fg_pool(masks)
    target = torch.zeros([renders.shape[0], 3], dtype=torch.float32, device=renders.device)
    sums, alpha = ops.brush_metrics(renders, target, masks, 10, True)
    s = pooled_scores(ops, sums, alpha, masks, fg_mask, n_fg)
    return {"BG_CLARITY_MEAN": s[0, 0].item(), "FG_OPACITY_MEDIAN": s[0, 1].item()}


def default_patch_width(r: int) -> int:
    """The window of ``compute_uniform_bg_lpips_metric`` for renders of side ``r`` (geom_metric.py:224-229): a quarter, else half
    where that stays at 64 or above, else 0.8 r."""
    p = r // 4
    if p < 64:
        p = r // 2
        if p < 64:
            p = int(0.8 * r)
    return p


def _i32(device, a) -> torch.Tensor:
    return torch.as_tensor(np.asarray(a, np.int32)).to(device)


def compute_uniform_bg_lpips_metric(renders, geom, lpips, patch_width=None, same_style=False, key_suffix=None, crops=None, ops=None):
    """({'LPIPS_UNIFORM_BG[_<key_suffix>]': value}, None) of ``renders`` [B,4,W,W] on the guidance ``geom`` [B,1,W,W], every image
    on its own drawing (geom_metric.py:207-262; the None stands for the debug image, which is not made).  ``lpips``: a
    ``perceptual.LPIPS``.  ``crops`` = (offset of the first window (row, column), of the second, permutation [B] or None): the
    draws of the call; None draws them as the reference does, from torch's global stream (one window pair per call, a permutation
    with ``same_style``).  ``ops``: whose ``bg_guidance`` / ``bg_mean_colors`` / ``metric_pairs`` prepare the pairs (``TileOps``:
    three launches); None: the torch restatement where the tensors are."""
    ops = TileOpsBase() if ops is None else ops
    key = "LPIPS_UNIFORM_BG" if key_suffix is None else f"LPIPS_UNIFORM_BG_{key_suffix}"
    b, r = renders.shape[0], renders.shape[-1]
    p = default_patch_width(r) if patch_width is None else int(patch_width)
    if crops is None:
        off0, off1 = (torch.randint(0, r - p + 1, (2,)).tolist() for _ in range(2))
        perm = torch.randperm(b).tolist() if same_style else None
    else:
        off0, off1, perm = crops
    guidance = ops.bg_guidance(geom.squeeze(1).to(torch.float32).contiguous())
    mean = ops.bg_mean_colors(renders, guidance)
    dev = renders.device
    x = ops.metric_pairs(renders, guidance, mean, _i32(dev, [list(off0)] * b).reshape(b, 2), _i32(dev, [list(off1)] * b).reshape(b, 2),
                         None if perm is None else _i32(dev, perm), p, True, True)
    return {key: lpips.pair_distance(x).mean().item()}, None


def compute_lpips_across_geo(renders, lpips, perm=None, ops=None):
    """{'LPIPS_ACROSS_GEO': value} of the renders [B,4,W,W] of ONE brush and colour (geom_metric.py:190-204): LPIPS between
    the on-white renders and a permutation of them (``perm`` [B]; None draws ``torch.randperm`` from the global stream)."""
    ops = TileOpsBase() if ops is None else ops
    b, r, dev = renders.shape[0], renders.shape[-1], renders.device
    perm = torch.randperm(b).tolist() if perm is None else perm
    zero = torch.zeros([b, 2], dtype=torch.int32, device=dev)
    x = ops.metric_pairs(renders, None, None, zero, zero, _i32(dev, perm), r, False, False)
    return {"LPIPS_ACROSS_GEO": lpips.pair_distance(x).mean().item()}


def compute_stitching_metrics(stitching_result, margin, lpips, ops=None):
    """{'STITCH_LPIPS', 'STITCH_L1'} of a ``RandomStitcher.generate_with_stitching`` dict (geom_metric.py:165-187): each 0.5 * (fake1
    against fake1_composite + fake2 against fake2_composite), all four images [N,3,R,R] cropped to ``[margin:R - 2 margin]`` on both
    axes first -- the reference's asymmetric crop, S = R - 3 margin wide --; LPIPS is the mean over the batch of the raw, unscaled
    images, L1 the mean over the N * 3 * S * S entries.  ``lpips``: a ``perceptual.LPIPS``.  The dict's images are composited already,
    so only the crop and the differences remain: torch where the tensors are, whatever ``ops`` (accepted like in the other
    functions); a library goes through ``BrushEvaluator.evaluate(stitch=)``, which composites, crops and sums in one launch."""
    m = int(margin)
    imgs = [stitching_result[key] for key in ("fake1", "fake2", "fake1_composite", "fake2_composite")]
    n, r = imgs[0].shape[0], imgs[0].shape[-1]
    if m < 0 or r - 3 * m < 1 or any(t.shape != imgs[0].shape for t in imgs):
        raise ValueError(f"compute_stitching_metrics: margin {margin} and images {[tuple(t.shape) for t in imgs]} do not fit")
    x = torch.cat([t[:, :, m:r - 2 * m, m:r - 2 * m].to(torch.float32) for t in imgs]).contiguous()
    d = lpips.pair_distance(x)
    l1 = (x[:2 * n] - x[2 * n:]).abs()
    return {"STITCH_LPIPS": (0.5 * (d[:n].mean() + d[n:].mean())).item(), "STITCH_L1": (0.5 * (l1[:n].mean() + l1[n:].mean())).item()}


# ---------------------------------------------------------------------------------------------------------------------
# a whole library
# ---------------------------------------------------------------------------------------------------------------------
def file_line(values, strip=True) -> str:
    """One line of the reference's metric files (``to_file_line``, metric_main.py:60-72): every value right-aligned in at least eight
    characters, separated by one blank."""
    cells = ["{}".format(v) for v in values]
    if strip:
        cells = ["".join(c.split()) for c in cells]
    return " ".join("{:>8}".format(c) for c in cells) + "\n"


def value_cells(values: Dict[str, float], keys: Sequence[str] = KEYS) -> List[str]:
    """The values in the order of ``keys``, four decimals, each as wide as its key (``ordered_dict_values``, metric_main.py:48-57)."""
    return [("{:>%d.4f}" % len(k)).format(values[k]) for k in keys]


@dataclasses.dataclass
class BrushScores:
    """The scores of a library's brushes (``BrushEvaluator.evaluate``), on the host: four float32 arrays [B] in the order of ``ids``,
    and, from a run with an LPIPS network, ``perceptual``: {key of ``PERCEPTUAL_KEYS``: float32 [B]}; from one with full-size
    drawings too, ``stitching``: {key of ``STITCH_KEYS``: float32 [B]}."""
    ids: List
    lab_e_percent: np.ndarray          # LAB_E%: share (in %) of the stroke's weight whose Lab distance to the picked colour exceeds lab_thresh
    lab_l2: np.ndarray                 # LAB_L2: mean over ALL pixels of weight * Lab distance
    bg_clarity_mean: np.ndarray        # BG_CLARITY_MEAN: 1 - mean alpha on sure background; NaN without background
    fg_opacity_median: np.ndarray      # FG_OPACITY_MEDIAN: lower median of alpha on the strokes; NaN without foreground
    perceptual: Optional[Dict[str, np.ndarray]] = None          # the three LPIPS numbers (lower = more uniform); None: not computed
    stitching: Optional[Dict[str, np.ndarray]] = None           # STITCH_L1, STITCH_LPIPS (lower = the seam shows less); None: not computed

    def keys(self) -> tuple:
        """The columns, sorted as the reference's files: ``KEYS``, and ``PERCEPTUAL_KEYS`` and ``STITCH_KEYS`` behind them when they
        were computed."""
        return KEYS + (() if self.perceptual is None else PERCEPTUAL_KEYS) + (() if self.stitching is None else STITCH_KEYS)

    def as_dict(self) -> Dict[str, np.ndarray]:
        d = {"BG_CLARITY_MEAN": self.bg_clarity_mean, "FG_OPACITY_MEDIAN": self.fg_opacity_median, "LAB_E%": self.lab_e_percent,
             "LAB_L2": self.lab_l2}
        if self.perceptual is not None:
            d.update({k: self.perceptual[k] for k in PERCEPTUAL_KEYS})
        if self.stitching is not None:
            d.update({k: self.stitching[k] for k in STITCH_KEYS})
        return d

    def summary(self) -> Dict[str, float]:
        """The mean over the brushes, as the reference's summary file (a NaN brush makes the mean NaN, as there)."""
        return {k: (float(np.mean(v.astype(np.float64))) if len(v) else float("nan")) for k, v in self.as_dict().items()}

    def rank(self, key: str) -> List:
        """The ids, best brush first: ascending for LAB_E%, LAB_L2 and the LPIPS numbers, descending for the clarity and the opacity;
        NaN last."""
        v = self.as_dict()[key].astype(np.float64)
        order = np.argsort(np.where(np.isnan(v), np.inf, -v if _HIGHER_IS_BETTER[key] else v), kind="stable")
        return [self.ids[i] for i in order.tolist()]

    def to_json(self) -> str:
        d = self.as_dict()
        return json.dumps({"ids": [str(i) for i in self.ids], "metrics": {k: [float(x) for x in d[k]] for k in self.keys()},
                           "summary": self.summary()})

    def write_reference_files(self, out_dir: str, prefix: str = ""):
        """``<prefix>style_metrics.txt`` (a line per brush) and ``<prefix>summary_metrics.txt`` in the reference's line format
        (metric_main.py:203-228): keys sorted, every cell right-aligned in at least eight characters.  Returns both paths."""
        os.makedirs(out_dir, exist_ok=True)
        style, summary = os.path.join(out_dir, f"{prefix}style_metrics.txt"), os.path.join(out_dir, f"{prefix}summary_metrics.txt")
        d, keys = self.as_dict(), self.keys()
        with open(style, "w") as f:
            f.write("SEED            " + file_line(keys))
            for i, sid in enumerate(self.ids):
                f.write("{:<15}".format(sid) + " " + file_line(value_cells({k: float(d[k][i]) for k in keys}, keys), strip=False))
        with open(summary, "w") as f:
            f.write(file_line(keys))
            f.write(file_line(value_cells(self.summary(), keys), strip=False))
        return style, summary


def default_colors(seed: int, n_brushes: int, rounds: int, k: int) -> np.ndarray:
    """[B, rounds, K, 3] float32: the colours the reference's loop draws (``RandomState(seed).random_tensor``, metrics/util.py:77-89 --
    a CPU ``torch.Generator`` seeded ``seed + 1`` -- asked for ``(K, 3)`` once per brush and round, brush-major, metric_main.py:153-156)."""
    gen = torch.Generator().manual_seed(int(seed) + 1)
    out = np.zeros([n_brushes, rounds, k, 3], np.float32)
    for b in range(n_brushes):
        for r in range(rounds):
            out[b, r] = torch.rand((k, 3), dtype=torch.float32, generator=gen).numpy()
    return out


def default_crops(seed: int, n_brushes: int, rounds: int, k: int, r: int, p: int) -> Dict[str, np.ndarray]:
    """The random plan of the perceptual scores for every (brush, round), from a CPU ``torch.Generator`` seeded ``seed + 2``.  Per
    unit, brush-major, in THIS order of draws:

        multi_off0, multi_off1   [B, rounds, 2] int32   the two windows (row, column) of LPIPS_UNIFORM_BG_multicolor, ``randint(0, r - p + 1, (2,))`` each
        same_off0, same_off1     [B, rounds, 2] int32   the two windows of LPIPS_UNIFORM_BG, likewise
        same_perm                [B, rounds, K] int32   its permutation of the K samples, ``randperm(k)`` (geom_metric.py:252)
        geo_perm                 [B, rounds, K] int32   the permutation of LPIPS_ACROSS_GEO, ``randperm(k)`` (geom_metric.py:201)

    One window pair serves the K samples of a unit: the reference's ``RandomCrop`` draws once per batched call (geom_metric.py:48-56,
    247-248).  Stated departure: the reference draws from the process-global streams, so no seed reproduces its draws; the
    distribution is the same."""
    if not 1 <= int(p) <= int(r):
        raise ValueError(f"default_crops: patch width {p} outside 1..{r}")
    gen = torch.Generator().manual_seed(int(seed) + 2)
    out = {name: np.zeros([n_brushes, rounds, 2], np.int32) for name in ("multi_off0", "multi_off1", "same_off0", "same_off1")}
    out.update({name: np.zeros([n_brushes, rounds, k], np.int32) for name in ("same_perm", "geo_perm")})
    for b in range(n_brushes):
        for j in range(rounds):
            for name in ("multi_off0", "multi_off1", "same_off0", "same_off1"):
                out[name][b, j] = torch.randint(0, r - p + 1, (2,), generator=gen).numpy()
            for name in ("same_perm", "geo_perm"):
                out[name][b, j] = torch.randperm(k, generator=gen).numpy()
    return out


CROP_KEYS = ("multi_off0", "multi_off1", "same_off0", "same_off1", "same_perm", "geo_perm")


@dataclasses.dataclass
class StitchSetup:
    """What ``BrushEvaluator.evaluate(stitch=)`` scores STITCH_* on: full-size drawings and the stitcher's two numbers
    (``RandomStitcher(crop_margin, min_overlap)``, stitching.py:194-200)."""
    drawings: np.ndarray             # [Ks,D,D] uint8, 0 = stroke, D above the engine's patch width
    margin: int = 10                 # crop_margin: how far a crop is inset before it is composited into the other; also the metric's crop
    min_overlap: int = 50


STITCH_PLAN_KEYS = ("crop1", "crop2", "positions1")


def default_stitch_plan(seed: int, n_brushes: int, rounds: int, k: int, r: int, d: int, margin: int = 10, min_overlap: int = 50) -> Dict[str, np.ndarray]:
    """The random plan of the stitching scores for every (brush, round), from a CPU ``torch.Generator`` seeded ``seed + 3`` (a stream
    of its own: ``default_colors`` and ``default_crops`` keep theirs).  Per unit, brush-major, in THIS order of draws:

        crop1        [B, rounds, 2] int32      (row, column) of the first r x r crop of the d x d drawings: ``randint(0, d - r + 1, (2,))``,
                                               the range of ``RandomCrop.get_params`` (metric_main.py:185)
        crop2        [B, rounds, 2] int32      of the second: per axis (row, then column) one ``randint`` over the INCLUSIVE range of
                                               ``CropHelper.gen_overlapping_square_crop`` (stitching.py:182-191): max(0, crop1 - radius) ..
                                               min(crop1 + radius, d - r - 1) with radius = r - margin - min_overlap - 1
        positions1   [B, rounds, K, 2] int32   the noise positions of the first render: ``randint(0, r - 1, (k, 2))`` (stitching.py:210)

    One crop pair serves the K samples of a unit: the reference's loop draws one per batch (metric_main.py:185-186).  Where the range of
    crop2 is empty (crop1 at d - r with radius 0; the reference's ``random.randint`` raises there) crop2 = crop1.  Stated departure,
    as for ``default_crops``: the reference draws from the process-global streams, so no seed reproduces its draws.  ValueError unless
    ``d > r`` and ``r - margin - min_overlap - 1 >= 0``."""
    r, d, margin, min_overlap = int(r), int(d), int(margin), int(min_overlap)
    radius = r - margin - min_overlap - 1
    if d <= r or radius < 0 or margin < 0 or min_overlap < 0:
        raise ValueError(f"default_stitch_plan: drawings of side {d} must exceed the patch width {r}, and r - margin - min_overlap - 1 = "
                         f"{radius} (margin {margin}, min_overlap {min_overlap}) must not be negative")
    gen = torch.Generator().manual_seed(int(seed) + 3)
    out = {"crop1": np.zeros([n_brushes, rounds, 2], np.int32), "crop2": np.zeros([n_brushes, rounds, 2], np.int32),
           "positions1": np.zeros([n_brushes, rounds, k, 2], np.int32)}
    for b in range(n_brushes):
        for j in range(rounds):
            c1 = torch.randint(0, d - r + 1, (2,), generator=gen).tolist()
            out["crop1"][b, j] = c1
            for axis in range(2):
                lo, hi = max(0, c1[axis] - radius), min(c1[axis] + radius, d - r - 1)
                out["crop2"][b, j, axis] = int(torch.randint(lo, hi + 1, (1,), generator=gen)) if hi >= lo else c1[axis]
            out["positions1"][b, j] = torch.randint(0, r - 1, (k, 2), generator=gen).numpy()
    return out


def _takes_keyword(fn, name: str) -> bool:
    """Whether the callback ``fn`` accepts the keyword ``name`` (by name or through ``**kwargs``)."""
    try:
        params = inspect.signature(fn).parameters.values()
    except (TypeError, ValueError):
        return False
    return any(q.name == name or q.kind is q.VAR_KEYWORD for q in params)


class BrushEvaluator:
    """Scores brushes on K guidance drawings.  ``drawings`` [K,R,R] uint8, 0 = stroke (R the engine's patch width): encoded once, and
    their evaluation masks built once (``ops.eval_masks``).  ``uvs_mapper``: a calibrated ``painting.StyleUVSMapper`` whose factors the
    renders use (one ``calibrate`` call per ``evaluate``); None renders without the clear-background mapping."""

    def __init__(self, ops, drawings, seed: int = 0, uvs_mapper=None):
        drawings = np.asarray(drawings)
        r = ops.patch_width
        if drawings.dtype != np.uint8 or drawings.ndim != 3 or drawings.shape[0] < 1 or drawings.shape[1:] != (r, r):
            raise ValueError(f"BrushEvaluator: uint8 drawings [K,{r},{r}] expected, got {drawings.dtype} {drawings.shape}")
        self.ops, self.seed, self.uvs_mapper = ops, int(seed), uvs_mapper
        geo = ops.to_device(drawings).to(torch.float32) / 255
        self.geom_feature = ops.encode(geo.unsqueeze(1))
        self.masks = ops.eval_masks(geo)
        self.fg_mask, self.n_fg = _fg_pool(self.masks)
        self._features: Dict = {}
        self._noise_set, self._noise_src = None, None
        self._guidance = None

    @property
    def k(self) -> int:
        return self.masks.geom.shape[0]

    def _geometry(self, nu: int):
        """The drawings' features for ``nu`` brushes, brush-major (sample u * K + d is unit u on drawing d)."""
        if nu == 1:
            return self.geom_feature
        if nu not in self._features:
            f = self.geom_feature
            self._features[nu] = f.repeated(nu) if hasattr(f, "repeated") else [x.repeat(nu, 1, 1, 1) for x in f]
        return self._features[nu]

    def _brush_noise(self, opts):
        """The noise set of a projected brush, as ``PaintingHelper._brush_noise``: one set, reloaded when the brush changes."""
        bufs = opts.custom_args.get("noise_buffers") if (opts.style_ws is not None and opts.custom_args) else None
        if not bufs:
            return None
        bn = self._noise_set
        if bn is None or bn.epoch is not bn.syn.packed:
            bn, self._noise_src = self.ops.brush_noise(), None
            if bn is None:
                return None
            self._noise_set = bn
        if bufs is not self._noise_src:
            bn.load(bufs)
            self._noise_src = bufs
        return bn

    @property
    def guidance(self):
        """The once-blurred guidance of the drawings (``ops.bg_guidance``), built at the first perceptual score."""
        if self._guidance is None:
            self._guidance = self.ops.bg_guidance(self.masks.geom)
        return self._guidance

    def perceptual_scores(self, lpips, renders: torch.Tensor, p: int, off0: torch.Tensor, off1: torch.Tensor,
                          perm: Optional[torch.Tensor] = None, geo_perm: Optional[torch.Tensor] = None):
        """(LPIPS_UNIFORM_BG [nu], LPIPS_ACROSS_GEO [nu] or None) on the device, of ``renders`` [nu*K,4,R,R], brush-major: each the
        mean over a unit's K pairs.  ``off0``, ``off1`` [nu,2] int32: a unit's two windows; ``perm`` [nu,K] int32: the unit's
        permutation of the second patches (None: none, the multicolour form); ``geo_perm`` [nu,K]: also score the across-drawing
        pairs.  Per metric: one launch for the pairs and one trunk pass over all 2 nu K images."""
        ops, k = self.ops, self.k
        nu = renders.shape[0] // k
        base = (torch.arange(nu, dtype=torch.int32, device=renders.device) * k).unsqueeze(1)
        src = lambda q: None if q is None else (base + q).reshape(-1).contiguous()
        mean = ops.bg_mean_colors(renders, self.guidance)
        x = ops.metric_pairs(renders, self.guidance, mean, off0.repeat_interleave(k, 0).contiguous(), off1.repeat_interleave(k, 0).contiguous(),
                             src(perm), p, True, True)
        uniform = lpips.pair_distance(x).view(nu, k).mean(dim=1)
        if geo_perm is None:
            return uniform, None
        zero = torch.zeros([nu * k, 2], dtype=torch.int32, device=renders.device)
        x = ops.metric_pairs(renders, None, None, zero, zero, src(geo_perm), renders.shape[-1], False, False)
        return uniform, lpips.pair_distance(x).view(nu, k).mean(dim=1)

    def score_renders(self, renders: torch.Tensor, targets: torch.Tensor, lab_thresh: float = 10) -> torch.Tensor:
        """[nu, 4] in the order of ``KEYS``, on the device: ``renders`` [nu*K,4,R,R] of nu brushes on the K drawings, brush-major,
        against the per-sample colours ``targets`` [nu*K,3].  Two launches (the sums, the median)."""
        sums, alpha = self.ops.brush_metrics(renders, targets, self.masks, lab_thresh, False)
        return pooled_scores(self.ops, sums, alpha, self.masks, self.fg_mask, self.n_fg)

    def evaluate(self, library, style_ids: Optional[Sequence] = None, rounds: int = 1, batch: int = 32, lab_thresh: float = 10,
                 colors=None, on_pass: Optional[Callable] = None, lpips=None, patch_width: Optional[int] = None, crops=None,
                 stitch: Optional[StitchSetup] = None, stitch_plan=None) -> BrushScores:
        """The scores of every brush of ``library`` (of ``style_ids``, in that order, if given), each the mean over ``rounds`` renders
        of the K drawings with fresh primary colours.  A unit is one brush in one round, K samples; ``floor(batch / K)`` units share a
        generator pass, brush-major; a brush that carries noise buffers gets passes of its own, with its noise set.  ``colors``
        [B, rounds, K, 3] in 0..1 replace the default stream (``default_colors(seed, ...)``, the reference's).  ``on_pass(units,
        renders, targets)`` (tests) sees every pass's [(brush index, round)], renders and colours before they are reduced.

        ``lpips`` (a ``perceptual.LPIPS``; the reference uses ``alex``): every pass is additionally scored for
        LPIPS_UNIFORM_BG_multicolor on the render it already makes, rendered once more with all-NaN user colours -- the brush's own
        colours (metric_main.py:172-173) -- and scored on that render for LPIPS_UNIFORM_BG and LPIPS_ACROSS_GEO; the scores carry
        ``perceptual``.  ``patch_width``: the windows' side (``default_patch_width(R)``); ``crops``: the plan of every unit
        (``default_crops(seed, ...)``).  A callback that takes the keyword ``own_renders`` (or ``**kwargs``) also sees the second
        render.

        ``stitch`` (a ``StitchSetup``; needs ``lpips``): STITCH_L1 and STITCH_LPIPS join them, the scores carry ``stitching``.  A unit
        is then also scored on the Ks full-size drawings: both crops of the unit's plan (``stitch_plan``, default
        ``default_stitch_plan(seed, ...)``) of every drawing are gathered (``ops.stitch_crops``) and encoded, rendered as raw images in
        ONE generator pass with noise positions ``positions2 = positions1 + (crop2 - crop1)`` (``ops.render_img``), composited, cropped
        and summed in one launch (``ops.stitch_pairs``), and the network runs once over the pass's 4 nu Ks images.  These passes are
        their own: ``floor(batch / (2 Ks))`` units share one, a brush with noise buffers again alone.  Stated departure: W+ brushes
        are scored like any other, where the reference skips them (metric_main.py:196-197, a TODO there).  A callback that takes the
        keyword ``stitch`` is also called once per such pass, as ``on_pass(units, None, None, stitch=info)`` with info = {"units",
        "crop1" [nu,2], "crop2" [nu,2], "positions1" [nu Ks,2], "positions2" [nu Ks,2], "fake" [2 nu Ks,3,R,R]} (the plan as host
        arrays, ``fake`` where it was rendered); its ordinary calls are as without ``stitch``.  Without ``stitch`` nothing changes."""
        ops, k = self.ops, self.k
        ids = list(library.get_style_ids() if style_ids is None else style_ids)
        rounds, per = int(rounds), max(1, int(batch) // k)
        if rounds < 1 or int(batch) < 1:
            raise ValueError(f"evaluate: rounds {rounds} and batch {batch} must be positive")
        from .painting import GanBrushOptions
        opts_list = []
        for sid in ids:
            opts_list.append(GanBrushOptions())
            library.set_style(sid, opts_list[-1])
        colors = default_colors(self.seed, len(ids), rounds, k) if colors is None else np.asarray(colors, np.float32)
        if colors.shape != (len(ids), rounds, k, 3):
            raise ValueError(f"evaluate: colours [{len(ids)},{rounds},{k},3] expected, got {colors.shape}")
        r_img = self.masks.geom.shape[-1]
        if lpips is not None:
            p = default_patch_width(r_img) if patch_width is None else int(patch_width)
            crops = default_crops(self.seed, len(ids), rounds, k, r_img, p) if crops is None else crops
            want = {name: (len(ids), rounds, k if name.endswith("perm") else 2) for name in CROP_KEYS}
            if any(name not in crops or tuple(np.shape(crops[name])) != shape for name, shape in want.items()):
                raise ValueError(f"evaluate: the crop plan needs {want}")
        if stitch is not None:
            if lpips is None:
                raise ValueError("evaluate: the stitching scores need an LPIPS network (lpips=)")
            sdraw = np.asarray(stitch.drawings)
            if sdraw.dtype != np.uint8 or sdraw.ndim != 3 or sdraw.shape[0] < 1 or sdraw.shape[1] != sdraw.shape[2] or sdraw.shape[1] <= r_img:
                raise ValueError(f"evaluate: uint8 stitch drawings [Ks,D,D] with D above the patch width {r_img} expected, got {sdraw.dtype} {sdraw.shape}")
            ks, d_full, margin = sdraw.shape[0], sdraw.shape[1], int(stitch.margin)
            if margin < 0 or r_img - 3 * margin < 1:
                raise ValueError(f"evaluate: stitch margin {margin} leaves no crop window of {r_img} - 3 * margin pixels")
            if stitch_plan is None:
                stitch_plan = default_stitch_plan(self.seed, len(ids), rounds, ks, r_img, d_full, margin, stitch.min_overlap)
            want = {"crop1": (len(ids), rounds, 2), "crop2": (len(ids), rounds, 2), "positions1": (len(ids), rounds, ks, 2)}
            if any(name not in stitch_plan or tuple(np.shape(stitch_plan[name])) != shape for name, shape in want.items()):
                raise ValueError(f"evaluate: the stitch plan needs {want}")
            splan = {name: np.asarray(stitch_plan[name]).astype(np.int64) for name in STITCH_PLAN_KEYS}
            if any(splan[name].size and (splan[name].min() < 0 or splan[name].max() > d_full - r_img) for name in ("crop1", "crop2")):
                raise ValueError(f"evaluate: the stitch plan's crops must lie in 0..{d_full - r_img}")
        if not ids:
            return BrushScores([], *(np.zeros([0], np.float32) for _ in range(4)),
                               perceptual=None if lpips is None else {key: np.zeros([0], np.float32) for key in PERCEPTUAL_KEYS},
                               stitching=None if stitch is None else {key: np.zeros([0], np.float32) for key in STITCH_KEYS})
        sf = self.uvs_mapper.calibrate(opts_list, batch) if self.uvs_mapper is not None else None
        ws = [ops.map_style(z=o.style_z, ws=o.style_ws) for o in opts_list]
        noisy = [bool(o.style_ws is not None and o.custom_args and o.custom_args.get("noise_buffers")) for o in opts_list]

        def split(per):
            """Lists of (brush, round), at most ``per`` each; a brush with noise never shares."""
            passes, cur = [], []
            for b in range(len(ids)):
                for r in range(rounds):
                    if cur and (len(cur) == per or noisy[b] != noisy[cur[-1][0]] or (noisy[b] and cur[-1][0] != b)):
                        passes.append(cur)
                        cur = []
                    cur.append((b, r))
            passes.append(cur)
            return passes
        passes = split(per)
        col_dev = ops.to_device(colors)                                   # [B, rounds, K, 3]
        if lpips is not None:                                             # the plan, unit-major: unit (b, r) is row b * rounds + r
            plan = {name: ops.to_device(np.ascontiguousarray(np.asarray(crops[name], np.int32).reshape(len(ids) * rounds, -1))) for name in CROP_KEYS}
            also_own = on_pass is not None and _takes_keyword(on_pass, "own_renders")
        scores, perc = [], []
        for units in passes:
            nu = len(units)
            bi = torch.tensor([b for b, _ in units], dtype=torch.int64)
            targets = torch.cat([col_dev[b, r] for b, r in units]).contiguous()                      # [nu*K, 3]
            user = torch.full([nu * k, 3, 3], float("nan"), dtype=torch.float32, device=targets.device)
            user[:, :, 0] = targets
            w = torch.cat([ws[b] for b, _ in units]).repeat_interleave(k, 0).contiguous()
            sfac = None if sf is None else sf[bi.to(sf.device)].repeat_interleave(k, 0).contiguous()
            noise = self._brush_noise(opts_list[units[0][0]]) if noisy[units[0][0]] else None
            renders = ops.render_rgba(w, self._geometry(nu), user, sfac, noise)
            if lpips is None:
                if on_pass is not None:
                    on_pass(units, renders, targets)
                scores.append(self.score_renders(renders, targets, lab_thresh))
                continue
            rows = torch.tensor([b * rounds + r for b, r in units], dtype=torch.int64, device=plan["multi_off0"].device)
            pl = {name: t[rows] for name, t in plan.items()}
            own = ops.render_rgba(w, self._geometry(nu), torch.full_like(user, float("nan")), sfac, noise)       # the brush's own colours
            if on_pass is not None:
                on_pass(units, renders, targets, **({"own_renders": own} if also_own else {}))
            scores.append(self.score_renders(renders, targets, lab_thresh))
            multi, _ = self.perceptual_scores(lpips, renders, p, pl["multi_off0"], pl["multi_off1"])
            same, geo = self.perceptual_scores(lpips, own, p, pl["same_off0"], pl["same_off1"], pl["same_perm"], pl["geo_perm"])
            perc.append(torch.stack([geo, same, multi], dim=1))            # (the order of PERCEPTUAL_KEYS)
        s = ops.to_host(torch.cat(scores).view(len(ids), rounds, 4).mean(dim=1).contiguous())
        perceptual = None
        if lpips is not None:
            q = ops.to_host(torch.cat(perc).view(len(ids), rounds, 3).mean(dim=1).contiguous())
            perceptual = {key: q[:, j].copy() for j, key in enumerate(PERCEPTUAL_KEYS)}
        stitching = None
        if stitch is not None:
            q = ops.to_host(self._stitch_scores(lpips, sdraw, margin, splan, ws, opts_list, noisy, split(max(1, int(batch) // (2 * ks))), rounds,
                                                on_pass if (on_pass is not None and _takes_keyword(on_pass, "stitch")) else None))
            stitching = {key: q[:, j].copy() for j, key in enumerate(STITCH_KEYS)}
        return BrushScores(ids, lab_e_percent=s[:, 2].copy(), lab_l2=s[:, 3].copy(), bg_clarity_mean=s[:, 0].copy(),
                           fg_opacity_median=s[:, 1].copy(), perceptual=perceptual, stitching=stitching)

    def _stitch_scores(self, lpips, sdraw: np.ndarray, margin: int, plan, ws, opts_list, noisy, passes, rounds: int, hook) -> torch.Tensor:
        """[B, 2] in the order of ``STITCH_KEYS``, on the device: the mean over the rounds of every brush's units, the passes as
        ``evaluate`` describes them.  ``plan``: int64 host arrays of ``STITCH_PLAN_KEYS``; ``ws``: every brush's styles."""
        ops, ks, r = self.ops, sdraw.shape[0], self.masks.geom.shape[-1]
        s = r - 3 * margin
        drawings = ops.to_device(np.ascontiguousarray(sdraw))
        out = []
        for units in passes:
            nu = len(units)
            n = nu * ks
            c1 = np.stack([plan["crop1"][b, j] for b, j in units])                                   # [nu, 2]
            c2 = np.stack([plan["crop2"][b, j] for b, j in units])
            p1 = np.concatenate([plan["positions1"][b, j] for b, j in units])                        # [n, 2], sample u * Ks + d
            p2 = p1 + np.repeat(c2 - c1, ks, axis=0)                                                 # CropHelper.position_delta
            rects = [stitch_rects((*c1[u], r, r), (*c2[u], r, r), margin) for u in range(nu)]
            rects_a = ops.to_device(np.ascontiguousarray(np.repeat(np.stack([a for a, _ in rects]), ks, axis=0)))
            rects_b = ops.to_device(np.ascontiguousarray(np.repeat(np.stack([b for _, b in rects]), ks, axis=0)))
            draw = ops.to_device(np.tile(np.arange(ks, dtype=np.int32), 2 * nu))
            offsets = ops.to_device(np.concatenate([np.repeat(c1, ks, axis=0), np.repeat(c2, ks, axis=0)]).astype(np.int32))
            feats = ops.encode(ops.stitch_crops(drawings, draw, offsets, r))                         # rows :n the first crops, n: the second
            w = torch.cat([ws[b] for b, _ in units]).repeat_interleave(ks, 0).repeat(2, 1, 1).contiguous()
            noise = self._brush_noise(opts_list[units[0][0]]) if noisy[units[0][0]] else None
            fake = ops.render_img(w, feats, ops.to_device(np.concatenate([p1, p2]).astype(np.int64)), noise)
            if hook is not None:
                hook(units, None, None, stitch={"units": list(units), "crop1": c1, "crop2": c2, "positions1": p1, "positions2": p2, "fake": fake})
            x, l1 = ops.stitch_pairs(fake, rects_a, rects_b, margin)
            dist = lpips.pair_distance(x)                                                            # [2n]: the first pairs, then the second
            lp = 0.5 * (dist[:n].view(nu, ks).mean(dim=1) + dist[n:].view(nu, ks).mean(dim=1))
            ab = 0.5 * (l1[:n].view(nu, ks).sum(dim=1) + l1[n:].view(nu, ks).sum(dim=1)) / float(ks * 3 * s * s)
            out.append(torch.stack([ab, lp], dim=1))
        return torch.cat(out).view(len(opts_list), rounds, 2).mean(dim=1).contiguous()
