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

Device work goes through ``tile_ops.TileOps`` (HIP kernels + the PyTorch-ROCm encoder).  The drivers here take ONE route whatever
ops they hold: there is no CPU fallback in them, and the tests inject stand-ins derived from ``tile_ops.TileOpsBase`` (oracle-backed, or
recording) to check the host logic and the sharded schedule on CPU.

This module holds the drivers: brush options, the UVS mapper, ``PaintingHelper`` and ``PaintSession``.  The host geometry and tiling
live in ``tiling``, the stroke model in ``strokes``, the device operations and their host restatements in ``tile_ops``; their public
names are imported here again, so ``painting.NAME`` keeps resolving for callers written before the split.
"""
from __future__ import annotations

import collections
import contextlib
import dataclasses
import os
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.distributed as dist

from .sharding import HaloExchange, shard_bounds, shard_sizes
# (what follows is also the re-export list: names this module used to define and does not use itself are imported all the same)
from .strokes import SEG_PITCH, StrokeList, flatten_splines_numpy, raster_segments_numpy, raster_strokes_numpy, strokes_bounds
from .tile_ops import (COMPOSE_MODES, PAINT_SLOT0, TileOps, TileOpsBase, canvas_view_numpy, on_white_torch, over_tiles_numpy,
                       stroke_counts_numpy)
from .tiling import (CELL_H, CELL_W, TileLayout, build_cells, cell_box, clear_outside, dirty_area_alpha, generate_stitching_crops,
                     pad_geo, prepare_geometry_image, read_geometry_image, stitching_grid, threshold_otsu, tiles_with_strokes)



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
# clear-background mapping (reference: StyleUVSMapper, forger/ui/mapper.py:16-72, 117-135)
# ------------------------------------------------------------------------------------------------
class StyleUVSMapper:
    """Per-style scale ``sfactor`` that stretches the background weight S of the triad so that clear background
    renders fully transparent; the remap itself (``_map_style_s``) is fused into the ToRGB launch
    (``nb_torgb_triad_f32(sfactor=...)``).  The reference calibrates on five bundled drawings at two stroke widths
    (``*_rad016.png`` / ``*_rad025.png``); they are data files of the reference, so the caller supplies them."""

    TOP_K = 15                   # the factor comes from the 15th largest background weight of a drawing (mapper.py:132)
    DEFAULT_BATCH = 32           # samples per generator pass of ``calibrate`` / ``catalogue``: floor(batch / K) brushes x K drawings

    def __init__(self, ops, cal_medium: Optional[np.ndarray] = None, cal_thick: Optional[np.ndarray] = None):
        self.ops = ops
        self.sfactors: Dict = {}
        self.geom_feature = self.bmask = None
        self._features: Dict = {}
        if cal_medium is not None:
            self.set_calibration(cal_medium, cal_thick)

    def set_calibration(self, cal_medium: np.ndarray, cal_thick: np.ndarray):
        """[k,R,R] uint8 drawings, 0 = stroke: medium strokes are rendered, thick ones define "surely background".  RuntimeError if
        a thick drawing leaves fewer than ``TOP_K`` background pixels (checked here, on the host, once: ``calibrate`` never needs the
        counts back from the device)."""
        cal_medium, cal_thick = np.asarray(cal_medium, np.uint8), np.asarray(cal_thick, np.uint8)
        background = (cal_thick.astype(np.float32) / np.float32(255) > np.float32(0.99)).reshape(cal_thick.shape[0], -1).sum(axis=1)
        for i, cnt in enumerate(background.tolist()):
            if cnt < self.TOP_K:
                raise RuntimeError(f"StyleUVSMapper: thick calibration drawing {i} leaves {cnt} background pixels; the factor is taken "
                                   f"from the {self.TOP_K} largest")
        geo = (self.ops.to_device(cal_medium).to(torch.float32) / 255).unsqueeze(1)
        self.geom_feature = self.ops.encode(geo)
        self.bmask = (self.ops.to_device(cal_thick).to(torch.float32) / 255).unsqueeze(1) > 0.99
        self.sfactors, self._features = {}, {}

    # -- rendering on the calibration drawings --
    def _need_calibration(self):
        if self.geom_feature is None:
            raise RuntimeError("StyleUVSMapper: no calibration drawings set (set_calibration)")

    def _geometry(self, nb: int, first_only: bool = False):
        """Geometry features of ``nb`` brushes on all K drawings (brush-major: sample b * K + d is brush b on drawing d), or of one
        brush on drawing 0 only (``[x[:1] for x in geom_feature]``, mapper.py:98).  Feature tensors are repeated; a provider the generator
        evaluates itself (``encoder.LazyGeometry``) repeats its drawings, and the encoder hands its output over the way it does for tiles."""
        if nb == 1 and not first_only:
            return self.geom_feature
        key = (nb, first_only)
        if key not in self._features:
            f = self.geom_feature
            if first_only:
                self._features[key] = f.sliced(0, 1) if hasattr(f, "sliced") else [x[:1] for x in f]
            else:
                self._features[key] = f.repeated(nb) if hasattr(f, "repeated") else [x.repeat(nb, 1, 1, 1) for x in f]
        return self._features[key]

    def _render(self, opts_list: Sequence, first_only: bool = False):
        """(img, debug data) of one un-positioned generator pass: every brush of ``opts_list`` on all K drawings, or on drawing 0 only.
        Without the brushes' noise buffers, as the reference (mapper.py:80-92)."""
        self._need_calibration()
        reps = 1 if first_only else self.bmask.shape[0]
        ws = torch.cat([self.ops.map_style(z=o.style_z, ws=o.style_ws) for o in opts_list])
        return self.ops.triad_debug(ws.repeat_interleave(reps, 0).contiguous(), self._geometry(len(opts_list), first_only))

    def _pass_sfactors(self, uvs: torch.Tensor, nb: int) -> torch.Tensor:
        """[nb] factors from the ``uvs`` [nb * K,3,R,R] of a pass: one selection launch on ``uvs[:, 2]`` in place, then the parent
        formula's own operations (minimum over the drawings, reciprocal)."""
        kth, _ = self.ops.masked_kth_largest(uvs[:, 2], self.bmask, self.TOP_K)
        return 1 / kth.view(nb, self.bmask.shape[0]).min(dim=1)[0]

    def _per_pass(self, batch: Optional[int]) -> int:
        batch = self.DEFAULT_BATCH if batch is None else int(batch)
        if batch < 1:
            raise ValueError(f"StyleUVSMapper: batch {batch} must be positive")
        return max(1, batch // self.bmask.shape[0])

    def calibrate(self, opts_list: Sequence, batch: Optional[int] = None) -> torch.Tensor:
        """The factors [B] of the brushes ``opts_list`` on the device, ``floor(batch / K)`` brushes per generator pass (batch 32 and the
        five drawings: six), the last pass ragged.  Nothing here waits for the device.  Fills the cache for every ``opts`` that has a
        ``style_id``."""
        self._need_calibration()
        opts_list, per = list(opts_list), self._per_pass(batch)
        parts = [self._pass_sfactors(self._render(opts_list[a:a + per])[1]["uvs"], len(opts_list[a:a + per]))
                 for a in range(0, len(opts_list), per)]
        sf = torch.cat(parts) if parts else torch.empty([0], dtype=torch.float32, device=self.bmask.device)
        self._remember(opts_list, sf)
        return sf

    def _remember(self, opts_list, sf: torch.Tensor):
        for i, o in enumerate(opts_list):
            if o.style_id is not None:
                self.sfactors[o.style_id] = sf[i]

    def get_sfactor(self, opts) -> torch.Tensor:
        if opts.style_id is not None and opts.style_id in self.sfactors:
            return self.sfactors[opts.style_id]
        return self.calibrate([opts])[0]

    # -- a brush's colours and icon (mapper.py:74-78, 94-115): the render on the first calibration drawing --
    @staticmethod
    def color_spec(colors) -> str:
        """'rgb(r,g,b):rgb(r,g,b):rgb(r,g,b)' of ``colors`` [1,3(rgb),3(k)] in -1..1, truncated as the reference does."""
        c = ((torch.as_tensor(colors)[0].detach().cpu() / 2 + 0.5) * 255).to(torch.uint8).numpy()
        return ":".join("rgb(%s)" % ",".join(str(int(x)) for x in c[:, i]) for i in range(3))

    @staticmethod
    def _icons(img: torch.Tensor, uvs: torch.Tensor, on_white: bool) -> torch.Tensor:
        """[n,R,R,3] uint8 where ``img`` is: the renders, over white by the background weight if asked, in the reference's operation order."""
        if on_white:
            img = img * (1 - uvs[:, 2:]) + uvs[:, 2:]
        return ((img.permute(0, 2, 3, 1) / 2 + 0.5) * 255).to(torch.uint8)

    def get_colors_raw(self, opts) -> torch.Tensor:
        """[1,3(rgb),3(k)] in -1..1: the three colours the generator gives the brush."""
        return self._render([opts], first_only=True)[1]["colors"]

    def get_colors(self, opts) -> str:
        return self.color_spec(self.get_colors_raw(opts))

    def get_brush_icon(self, opts, on_white: bool = True) -> np.ndarray:
        """[R,R,3] uint8: the brush on the first calibration drawing."""
        img, dbg = self._render([opts], first_only=True)
        return self.ops.to_host(self._icons(img, dbg["uvs"], on_white)[0].contiguous())

    # -- a whole library --
    def catalogue(self, library, style_ids: Optional[Sequence] = None, batch: Optional[int] = None, on_white: bool = True,
                  icon_k: int = 1) -> "BrushCatalogue":
        """Icon, colours and factor of every brush of ``library`` (of ``style_ids``, in that order, if given): one generator pass per
        ``floor(batch / K)`` brushes serves all three -- sample b * K of a pass is brush b on drawing 0 (colours, icon), its K samples
        give the factor.  ``icon_k`` in 1..16, a divisor of R, reduces the icons on the device (``ops.canvas_view`` on the icons stacked
        as an opaque canvas); only the reduced icons, the colours and the factors are copied to the host.  Fills the factor cache like
        ``calibrate``."""
        self._need_calibration()
        R, K, icon_k = self.ops.patch_width, self.bmask.shape[0], int(icon_k)
        if not 1 <= icon_k <= 16 or R % icon_k:
            raise ValueError(f"catalogue: icon_k {icon_k} must lie in 1..16 and divide the patch width {R}")
        ids = list(library.get_style_ids() if style_ids is None else style_ids)
        opts_list, per = [], self._per_pass(batch)
        for sid in ids:
            opts_list.append(GanBrushOptions())
            library.set_style(sid, opts_list[-1])
        sf, colors, icons = [], [], []
        for a in range(0, len(ids), per):
            nb = len(opts_list[a:a + per])
            img, dbg = self._render(opts_list[a:a + per])
            sf.append(self._pass_sfactors(dbg["uvs"], nb))
            colors.append(dbg["colors"][::K])
            icons.append(self._icons(img[::K], dbg["uvs"][::K], on_white))
        dev, r = self.bmask.device, R // icon_k
        if not ids:
            return BrushCatalogue([], [], np.zeros([0, 3, 3], np.float32), [], np.zeros([0], np.float32), np.zeros([0, r, r, 3], np.uint8))
        sf, colors, icons = torch.cat(sf), torch.cat(colors).contiguous(), torch.cat(icons)
        self._remember(opts_list, sf)
        if icon_k > 1:
            small = []
            for a in range(0, len(ids), 64):                       # (groups keep the view's window within its launch limits)
                grp = icons[a:a + 64]
                nb = grp.shape[0]
                canvas = torch.cat([grp, torch.full([nb, R, R, 1], 255, dtype=torch.uint8, device=dev)], dim=3).reshape(nb * R, R, 4)
                small.append(self.ops.canvas_view(canvas.contiguous(), 0, 0, nb * R, R, icon_k)[..., :3].reshape(nb, r, r, 3))
            icons = torch.cat(small)
        colors = self.ops.to_host(colors)
        return BrushCatalogue(ids, opts_list, colors, [self.color_spec(colors[i:i + 1]) for i in range(len(ids))],
                              self.ops.to_host(sf.contiguous()), self.ops.to_host(icons.contiguous()))


@dataclasses.dataclass
class BrushCatalogue:
    """What a brush picker shows for a library (``StyleUVSMapper.catalogue``), on the host."""
    ids: List
    opts: List[GanBrushOptions]        # what ``library.set_style`` produced: paint with these (a ``rand<N>`` id cannot be drawn again)
    colors_raw: np.ndarray             # [B,3(rgb),3(k)] float32 in -1..1
    color_specs: List[str]             # 'rgb(r,g,b):rgb(r,g,b):rgb(r,g,b)' per brush
    sfactors: np.ndarray               # [B] float32 clear-background factors
    icons: np.ndarray                  # [B, R/icon_k, R/icon_k, 3] uint8

    def to_json(self) -> str:
        import json
        return json.dumps({"ids": [str(i) for i in self.ids], "color_specs": list(self.color_specs),
                           "sfactors": [float(s) for s in self.sfactors]})

    def sheet(self, cols: int = 10) -> np.ndarray:
        """The icons side by side, ``cols`` per row, on white: [rows * r, cols * r, 3] uint8."""
        n, r = self.icons.shape[0], self.icons.shape[1]
        cols = max(1, min(int(cols), max(n, 1)))
        rows = max(1, -(-n // cols))
        out = np.full((rows * r, cols * r, 3), 255, np.uint8)
        for i in range(n):
            y, x = (i // cols) * r, (i % cols) * r
            out[y:y + r, x:x + r] = self.icons[i]
        return out

    def save_sheet(self, path: str, cols: int = 10) -> str:
        from PIL import Image
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        Image.fromarray(self.sheet(cols)).save(path)
        return path


def crop_drawing(ops, canvas: torch.Tensor, m: int, size_hw, on_white: bool) -> np.ndarray:
    """The [h0, w0] drawing at (m, m) of the padded RGBA canvas, as numpy: RGBA, or 3 channels composited on white.  Cropped (and
    composited) where the canvas is: only the answer crosses PCIe."""
    h0, w0 = size_hw
    return ops.to_host(ops.composite_on_white(canvas, m, m, h0, w0) if on_white else canvas[m:m + h0, m:m + w0].contiguous())


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
        layout = TileLayout.of(crops, R, int(crop_margin), self.down_factor)
        rgba_all = self._schedule(geom_padded.reshape(H, W), crops, layout.floored, crops, opts, crop_margin)
        if rgba_all is None:
            return None
        if out_canvas is None:
            out_canvas = torch.zeros([H, W, 4], dtype=torch.uint8, device=ops.device)
        ops.paste(out_canvas, rgba_all, *layout.device_args(ops.to_device, H, W))
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
        pad, tile with 2*crop_margin overlap, stylize every tile, paste, composite, crop.  Rank 0 returns the image.

        This is the independent HOST restatement of that loop -- ``pad_geo``, ``generate_stitching_crops``, the crop and the torch
        on-white expression, none of the preparation kernels or their ``TileOpsBase`` counterparts -- and stays apart from
        ``_paint_padded`` on purpose: it is what ``paint_drawing`` and ``paint_strokes`` are held to, byte for byte."""
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
            result = on_white_torch(result)
        out = to_host(result.contiguous())
        if not return_full:
            return out
        return out, to_host(canvas), crops, padded

    def paint_drawing(self, img: np.ndarray, opts: GanBrushOptions, crop_margin: int = 10, stitching_mode: str = "all",
                      on_white: bool = False, return_full: bool = False):
        """``paint_image(prepare_geometry_image(img), ...)`` with the preparation on the device: the decoded drawing (uint8 [H,W],
        [H,W,3] or [H,W,4]) is uploaded once, thresholded straight into the padded geometry (``nb_geom_prepare_u8``), the tiles are
        picked from per-tile stroke counts (``nb_tile_stroke_counts_u8``), the schedule runs on the device-resident geometry and the
        result is cropped / composited on white on the device.  Same bytes as the host route ``paint_image``.  The CPU stand-ins of the
        tests take this very route, with the host restatements of ``TileOpsBase`` in place of the kernels."""
        ops, R, m = self.ops, self.patch_width, int(crop_margin)
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
            tile_yx = [(row * stride, col * stride) for row in range(nrows) for col in range(ncols)]
        else:
            tile_yx = tiles_with_strokes(ops.to_host(ops.stroke_counts(padded, R, stride, nrows, ncols)), stride).tolist()
        crops = [(y, x, R, R) for y, x in tile_yx]                                                  # row-major, as the host loop
        self.make_new_canvas(ph, pw, self.feature_blending_level)
        canvas = self.render_tiles(padded, crops, opts, crop_margin=m)
        if canvas is None:
            return None
        out = crop_drawing(ops, canvas, m, (h0, w0), on_white)
        if not return_full:
            return out
        return out, ops.to_host(canvas), crops, ops.to_host(padded)[..., None]

    def paint_strokes(self, strokes: StrokeList, size_hw, opts: GanBrushOptions, crop_margin: int = 10, stitching_mode: str = "all",
                      on_white: bool = False, return_full: bool = False, subdiv: int = 8):
        """``paint_drawing`` from strokes instead of a raster: the strokes of a [h, w] = ``size_hw`` drawing (``StrokeList``: points and
        radii, kilobytes) are uploaded, splines are cut into segments and all segments rasterised straight into the padded geometry on
        the device (``nb_spline_flatten_f32``, ``nb_raster_segments_u8``); tile picks, schedule, crop and on-white follow as in
        ``paint_drawing``.  Strokes are clipped to the drawing: the padding around it stays background.  Same bytes as
        ``paint_image`` on the rasterised strokes.  Every rank of a sharded run rasterises the stroke list itself."""
        ops, R, m = self.ops, self.patch_width, int(crop_margin)
        h0, w0 = int(size_hw[0]), int(size_hw[1])
        if h0 < 1 or w0 < 1:
            raise ValueError(f"paint_strokes: bad canvas size {size_hw}")
        nrows, ncols, stride, ph, pw = stitching_grid(h0 + m, w0 + m, R, 2 * m)
        padded = ops.raster_strokes(strokes, (ph, pw), (m, m), subdiv=subdiv)
        clear_outside(padded, m, m + h0, m, m + w0)
        return self._paint_padded(padded, (h0, w0), (nrows, ncols, stride), opts, m, stitching_mode, on_white, return_full)


# ------------------------------------------------------------------------------------------------
# the paint session: a canvas that stays on the device, strokes added one call at a time, each with its own brush
# ------------------------------------------------------------------------------------------------
EMPTY_BOX = (0, 0, 0, 0)


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
        geom = ops.raster_strokes(strokes, (sh, sw), (m - gy0, m - gx0), subdiv=subdiv)
        clear_outside(geom, m - gy0, m + h0 - gy0, m - gx0, m + w0 - gx0)
        geom_yx = tiles_with_strokes(ops.to_host(ops.stroke_counts(geom, R, stride, nr, nc)), stride)
        if geom_yx.shape[0] == 0:
            return EMPTY_BOX
        self.last_tiles = geom_yx.shape[0]
        crops = geom_yx + np.array([gy0, gx0], np.int64)
        df = helper.down_factor
        layout = TileLayout.of(crops, R, m, df)
        self._reset_feature_mask()
        rgba = helper._schedule(geom, geom_yx, layout.floored, crops, opts, m)
        if helper.feature_blending_level > 0:
            a, bres = layout.floored // df, R // df
            self._mask_seen = helper.mask
            self._mask_rect = (int(a[:, 0].min()), int(a[:, 1].min()), int(a[:, 0].max()) + bres, int(a[:, 1].max()) + bres)
        box = layout.box(ph, pw)                                           # around the interiors: what the paste of render_tiles writes
        self._undo.append((box, self.canvas[box[0]:box[2], box[1]:box[3]].clone()))
        ops.over_tiles(self.canvas, rgba, *layout.device_args(ops.to_device, ph, pw), box=box, mode=COMPOSE_MODES[mode], opacity=int(opacity))
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
        return crop_drawing(self.ops, self.canvas, self.crop_margin, self.size_hw, on_white)
