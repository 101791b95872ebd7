"""Brush scores: the four numbers the reference reports per brush (``paint_engine_metric_loop``, forger/metrics/metric_main.py:105-236),
computed where the renders are.

    LAB_E%, LAB_L2                       how well the stroke takes the user's primary colour, in CIE Lab
                                         (``compute_lab_metrics``, forger/metrics/color_metric.py:29-70)
    BG_CLARITY_MEAN, FG_OPACITY_MEDIAN   how clear the background and how opaque the stroke is
                                         (``compute_transparency_metrics``, forger/metrics/geom_metric.py:126-162)

The three functions keep the reference's signatures and keys, so a caller of the reference can switch; ``BrushEvaluator`` scores a
whole library in batches: ``floor(batch / K)`` brushes share a generator pass on the K drawings, ``ops.brush_metrics`` reduces the
pass's renders to four sums per image in one launch, and the pooled median is ``ops.masked_kth_largest`` on the alpha planes it
leaves.  Nothing is copied to the host until the ``BrushScores`` are assembled.  The reference's LPIPS-based items (``BG_LPIPS*``,
``STITCH_*``, ``LPIPS_ACROSS_GEO``) need a pretrained network and are not part of this module.
"""
from __future__ import annotations

import dataclasses
import json
import os
from typing import Callable, Dict, List, Optional, Sequence

import numpy as np
import torch

from .tile_ops import EvalMasks, TileOpsBase, lab_deltas_torch

KEYS = ("BG_CLARITY_MEAN", "FG_OPACITY_MEDIAN", "LAB_E%", "LAB_L2")          # sorted, the column order of the reference's files
_HIGHER_IS_BETTER = {"BG_CLARITY_MEAN": True, "FG_OPACITY_MEDIAN": True, "LAB_E%": False, "LAB_L2": False}


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


def value_cells(values: Dict[str, float]) -> List[str]:
    """The values in the order of ``KEYS``, four decimals, each as wide as its key (``ordered_dict_values``, metric_main.py:48-57)."""
    return [("{:>%d.4f}" % len(k)).format(values[k]) for k in KEYS]


@dataclasses.dataclass
class BrushScores:
    """The scores of a library's brushes (``BrushEvaluator.evaluate``), on the host: four float32 arrays [B] in the order of ``ids``."""
    ids: List
    lab_e_percent: np.ndarray          # LAB_E%: share (in %) of the stroke's weight whose Lab distance to the picked colour exceeds lab_thresh
    lab_l2: np.ndarray                 # LAB_L2: mean over ALL pixels of weight * Lab distance
    bg_clarity_mean: np.ndarray        # BG_CLARITY_MEAN: 1 - mean alpha on sure background; NaN without background
    fg_opacity_median: np.ndarray      # FG_OPACITY_MEDIAN: lower median of alpha on the strokes; NaN without foreground

    def as_dict(self) -> Dict[str, np.ndarray]:
        return {"BG_CLARITY_MEAN": self.bg_clarity_mean, "FG_OPACITY_MEDIAN": self.fg_opacity_median, "LAB_E%": self.lab_e_percent,
                "LAB_L2": self.lab_l2}

    def summary(self) -> Dict[str, float]:
        """The mean over the brushes, as the reference's summary file (a NaN brush makes the mean NaN, as there)."""
        return {k: (float(np.mean(v.astype(np.float64))) if len(v) else float("nan")) for k, v in self.as_dict().items()}

    def rank(self, key: str) -> List:
        """The ids, best brush first: ascending for LAB_E% and LAB_L2, descending for the clarity and the opacity; NaN last."""
        v = self.as_dict()[key].astype(np.float64)
        order = np.argsort(np.where(np.isnan(v), np.inf, -v if _HIGHER_IS_BETTER[key] else v), kind="stable")
        return [self.ids[i] for i in order.tolist()]

    def to_json(self) -> str:
        d = self.as_dict()
        return json.dumps({"ids": [str(i) for i in self.ids], "metrics": {k: [float(x) for x in d[k]] for k in KEYS},
                           "summary": self.summary()})

    def write_reference_files(self, out_dir: str, prefix: str = ""):
        """``<prefix>style_metrics.txt`` (a line per brush) and ``<prefix>summary_metrics.txt`` in the reference's line format
        (metric_main.py:203-228): keys sorted, every cell right-aligned in at least eight characters.  Returns both paths."""
        os.makedirs(out_dir, exist_ok=True)
        style, summary = os.path.join(out_dir, f"{prefix}style_metrics.txt"), os.path.join(out_dir, f"{prefix}summary_metrics.txt")
        d = self.as_dict()
        with open(style, "w") as f:
            f.write("SEED            " + file_line(KEYS))
            for i, sid in enumerate(self.ids):
                f.write("{:<15}".format(sid) + " " + file_line(value_cells({k: float(d[k][i]) for k in KEYS}), strip=False))
        with open(summary, "w") as f:
            f.write(file_line(KEYS))
            f.write(file_line(value_cells(self.summary()), strip=False))
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

    def score_renders(self, renders: torch.Tensor, targets: torch.Tensor, lab_thresh: float = 10) -> torch.Tensor:
        """[nu, 4] in the order of ``KEYS``, on the device: ``renders`` [nu*K,4,R,R] of nu brushes on the K drawings, brush-major,
        against the per-sample colours ``targets`` [nu*K,3].  Two launches (the sums, the median)."""
        sums, alpha = self.ops.brush_metrics(renders, targets, self.masks, lab_thresh, False)
        return pooled_scores(self.ops, sums, alpha, self.masks, self.fg_mask, self.n_fg)

    def evaluate(self, library, style_ids: Optional[Sequence] = None, rounds: int = 1, batch: int = 32, lab_thresh: float = 10,
                 colors=None, on_pass: Optional[Callable] = None) -> BrushScores:
        """The scores of every brush of ``library`` (of ``style_ids``, in that order, if given), each the mean over ``rounds`` renders
        of the K drawings with fresh primary colours.  A unit is one brush in one round, K samples; ``floor(batch / K)`` units share a
        generator pass, brush-major; a brush that carries noise buffers gets passes of its own, with its noise set.  ``colors``
        [B, rounds, K, 3] in 0..1 replace the default stream (``default_colors(seed, ...)``, the reference's).  ``on_pass(units,
        renders, targets)`` (tests) sees every pass's [(brush index, round)], renders and colours before they are reduced."""
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
        if not ids:
            return BrushScores([], *(np.zeros([0], np.float32) for _ in range(4)))
        sf = self.uvs_mapper.calibrate(opts_list, batch) if self.uvs_mapper is not None else None
        ws = [ops.map_style(z=o.style_z, ws=o.style_ws) for o in opts_list]
        noisy = [bool(o.style_ws is not None and o.custom_args and o.custom_args.get("noise_buffers")) for o in opts_list]
        passes, cur = [], []                                              # lists of (brush, round); a brush with noise never shares
        for b in range(len(ids)):
            for r in range(rounds):
                if cur and (len(cur) == per or noisy[b] != noisy[cur[-1][0]] or (noisy[b] and cur[-1][0] != b)):
                    passes.append(cur)
                    cur = []
                cur.append((b, r))
        passes.append(cur)
        col_dev = ops.to_device(colors)                                   # [B, rounds, K, 3]
        scores = []
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
            if on_pass is not None:
                on_pass(units, renders, targets)
            scores.append(self.score_renders(renders, targets, lab_thresh))
        s = ops.to_host(torch.cat(scores).view(len(ids), rounds, 4).mean(dim=1).contiguous())
        return BrushScores(ids, lab_e_percent=s[:, 2].copy(), lab_l2=s[:, 3].copy(), bg_clarity_mean=s[:, 0].copy(),
                           fg_opacity_median=s[:, 1].copy())
