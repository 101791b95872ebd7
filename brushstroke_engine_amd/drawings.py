"""Synthetic stroke drawings: seeded random centripetal Catmull-Rom patches, K at a time (``csrc/nb_drawings.hip``).

What the reference makes with ``scripts/create_splines.py`` -- random control points (``forger/core/curve.py:98-116``), a thickness from
``forger/util/spline_dist.py`` or a fixed list of radii, the curve drawn and dilated on the host -- from a seed, on the device:
``SplineSynth.batch`` runs ``nb_synth_spline_counts`` (host integers) -> ``nb_synth_spline_ctrl_f32`` -> ``nb_spline_flatten_f32`` ->
``nb_raster_batch_u8`` with nothing synchronised.  ``include/neube_hip.h`` states the draws; the numpy functions here restate them in
float64: they are what the tests hold the kernels to, and what a CPU device runs.  ``load_drawings`` / ``load_calibration`` let every
tool take ``synth:...`` where it takes a file of drawings."""
from __future__ import annotations

import ctypes
import dataclasses
import os
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .strokes import SEG_PITCH, StrokeList, flatten_splines_numpy, raster_segments_numpy

MASK32, MASK64 = 0xFFFFFFFF, (1 << 64) - 1
SPLN = 0x53504C4E            # counter word 1 of every draw of a drawing
TRIES = 8                    # Gaussian thickness tries: draws P(1) .. P(8)
CTRL_DRAW0 = 16              # control point i is draw P(16 + i)
REFERENCE_WIDTH = 256        # the patch width the reference's thickness numbers are for
F1_1, F0_05 = float(np.float32(1.1)), float(np.float32(0.05))        # the kernel's fp32 constants, widened
SUBDIV = 8                   # pieces per span, the default of TileOps.raster_strokes
MIN_BACKGROUND = 15          # StyleUVSMapper.TOP_K: background pixels a thick calibration drawing must leave
CALIBRATION_K, CALIBRATION_RADII, CALIBRATION_RETRIES = 5, (16, 25), 16


@dataclasses.dataclass(frozen=True)
class SplineSpec:
    """``struct NbSplineSpec``: how many control points, where, how thick.  The defaults are the reference's flags: 4..15 points,
    ``rand * 2.2 - 1`` placement (``mode="cells"`` is ``--smart_sampling``), a Gaussian mixture with centres 6, 10, sigmas 2, 3 and
    weights 6 : 10 (``--thick_dist gauss``); ``thick="range"`` is ``--thick_dist rand`` (1..30), ``thick="fixed"`` one ``--use_radii``
    radius.  Thickness numbers are pixels; the reference's are for 256-pixel patches (``scaled``)."""
    pts_min: int = 4
    pts_max: int = 15
    mode: str = "uniform"
    thick: str = "mixture"
    radius: float = 16.0
    rmin: int = 1
    rmax: int = 30
    centers: Tuple[float, ...] = (6.0, 10.0)
    sigmas: Tuple[float, ...] = (2.0, 3.0)
    weights: Tuple[float, ...] = (6.0, 10.0)

    def __post_init__(self):
        if not 4 <= int(self.pts_min) <= int(self.pts_max) <= _lib.NB_SYNTH_MAX_POINTS:
            raise ValueError(f"SplineSpec: pts {self.pts_min}..{self.pts_max} outside 4 <= min <= max <= {_lib.NB_SYNTH_MAX_POINTS}")
        if self.mode not in _lib.NB_SPLINE_MODES:
            raise ValueError(f"SplineSpec: mode {self.mode!r} is none of {sorted(_lib.NB_SPLINE_MODES)}")
        if self.thick not in _lib.NB_THICK_MODES:
            raise ValueError(f"SplineSpec: thick {self.thick!r} is none of {sorted(_lib.NB_THICK_MODES)}")
        if self.thick == "fixed" and not (np.isfinite(self.radius) and self.radius >= 0):
            raise ValueError(f"SplineSpec: radius {self.radius}")
        if self.thick == "range" and not 0 <= int(self.rmin) <= int(self.rmax) <= 1 << 20:
            raise ValueError(f"SplineSpec: radius range {self.rmin}..{self.rmax}")
        if self.thick == "mixture":
            n = len(self.centers)
            if not (1 <= n <= _lib.NB_SYNTH_MAX_MIX and len(self.sigmas) == n and len(self.weights) == n):
                raise ValueError(f"SplineSpec: 1..{_lib.NB_SYNTH_MAX_MIX} centres with as many sigmas and weights expected")
            if min(self.sigmas) < 0 or min(self.weights) < 0 or not sum(self.weights) > 0:
                raise ValueError("SplineSpec: sigmas and weights must not be negative, and some weight positive")

    def scaled(self, r: int) -> "SplineSpec":
        """The thickness parameters multiplied by ``r / 256`` (integer ranges and the fixed radius rounded; a range keeps at least 1)."""
        f = float(r) / REFERENCE_WIDTH
        return dataclasses.replace(self, radius=float(np.rint(self.radius * f)), rmin=max(int(np.rint(self.rmin * f)), min(self.rmin, 1)),
                                   rmax=max(int(np.rint(self.rmax * f)), 1), centers=tuple(c * f for c in self.centers),
                                   sigmas=tuple(s * f for s in self.sigmas))

    def fixed(self, radius: float) -> "SplineSpec":
        return dataclasses.replace(self, thick="fixed", radius=float(radius))

    def cdf(self) -> np.ndarray:
        """Normalised cumulative weights, float32, last entry 1."""
        c = (np.cumsum(np.asarray(self.weights, np.float64)) / float(np.sum(np.asarray(self.weights, np.float64)))).astype(np.float32)
        c[-1] = 1.0
        return c

    def to_c(self) -> _lib.NbSplineSpec:
        s = _lib.NbSplineSpec(pts_min=int(self.pts_min), pts_max=int(self.pts_max), mode=_lib.NB_SPLINE_MODES[self.mode],
                              thick_mode=_lib.NB_THICK_MODES[self.thick], radius=float(self.radius), rmin=int(self.rmin), rmax=int(self.rmax),
                              n_mix=len(self.centers))
        if self.thick == "mixture":
            for i, (c, g, p) in enumerate(zip(self.centers, self.sigmas, self.cdf())):
                s.center[i], s.sigma[i], s.cdf[i] = float(c), float(g), float(p)
        return s


# ---------------------------------------------------------------------------------------------------------------------
# the draws in numpy: Philox4x32-10 on uint64 arrays (the constants of nb_noise_seeded_f32), float64 from the same integers
# ---------------------------------------------------------------------------------------------------------------------
def _philox(counter, key):
    c = list(np.broadcast_arrays(*[np.asarray(v, dtype=np.uint64) & np.uint64(MASK32) for v in counter]))
    k0, k1 = int(key[0]) & MASK32, int(key[1]) & MASK32
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & np.uint64(MASK32), (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & np.uint64(MASK32)]
        k0, k1 = (k0 + 0x9E3779B9) & MASK32, (k1 + 0xBB67AE85) & MASK32
    return c


def _draw(j, s, seed):
    """P(j) of the drawings with sample numbers ``s`` (uint64 array): four uint64 arrays of 32-bit values, broadcast over j and s."""
    s = np.asarray(s, np.uint64)
    seed = int(seed) & MASK64
    return _philox((j, SPLN, s & np.uint64(MASK32), s >> np.uint64(32)), (seed & MASK32, seed >> 32))


def _unit(x):
    return (x >> np.uint64(8)).astype(np.float64) * 2.0 ** -24


def _samples(offset, k):
    return (np.arange(int(k), dtype=np.uint64) + np.uint64(int(offset) & MASK64))          # (uint64 addition wraps)


def synth_counts_numpy(spec: SplineSpec, seed: int, offset: int, k: int) -> np.ndarray:
    """``nb_synth_spline_counts``: [k] int32 control points per drawing."""
    x0 = _draw(0, _samples(offset, k), seed)[0]
    return (int(spec.pts_min) + (x0 % np.uint64(spec.pts_max - spec.pts_min + 1)).astype(np.int64)).astype(np.int32)


def thickness_tries_numpy(spec: SplineSpec, seed: int, offset: int, k: int) -> np.ndarray:
    """[k, 8] float64: ``v = center[c] + sigma[c] * z`` of the eight Gaussian tries of every drawing (mixture mode), on the fp32
    centres and sigmas the kernel reads: the values whose distance to -0.5 and to the half-integers decides acceptance and rounding."""
    s = _samples(offset, k)
    c = np.minimum(np.searchsorted(spec.cdf().astype(np.float64), _unit(_draw(0, s, seed)[1]), side="right"), len(spec.centers) - 1)
    t = _draw(np.arange(1, 1 + TRIES, dtype=np.uint64)[None, :], s[:, None], seed)
    u1 = ((t[0] >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24
    ang = (t[1] >> np.uint64(8)).astype(np.int64)                                       # angle = pi t / 2^23, the quadrant reduced in integers
    quad, frac = ang >> 22, (ang & ((1 << 22) - 1)).astype(np.float64) * (np.pi / 2 ** 23)
    cos = np.choose(quad, [np.cos(frac), -np.sin(frac), -np.cos(frac), np.sin(frac)])
    z = np.sqrt(-2.0 * np.log(u1)) * cos
    center = np.asarray(spec.centers, np.float32).astype(np.float64)[c]
    sigma = np.asarray(spec.sigmas, np.float32).astype(np.float64)[c]
    return center[:, None] + sigma[:, None] * z


def synth_radii_numpy(spec: SplineSpec, seed: int, offset: int, k: int) -> np.ndarray:
    """[k] float64 radii (before ``r_eff``): the fixed radius, the integer-range draw, or the first accepted Gaussian try rounded
    half to even (``rintf``); 0 when none of the eight is accepted."""
    if spec.thick == "fixed":
        return np.full(int(k), float(np.float32(spec.radius)))
    if spec.thick == "range":
        x2 = _draw(0, _samples(offset, k), seed)[2]
        return (int(spec.rmin) + (x2 % np.uint64(spec.rmax - spec.rmin + 1)).astype(np.int64)).astype(np.float64)
    v = thickness_tries_numpy(spec, seed, offset, k)
    ok = v >= -0.5
    first = np.argmax(ok, axis=1)
    return np.where(ok.any(axis=1), np.rint(v[np.arange(int(k)), first]), 0.0)


def synth_ctrl_numpy(spec: SplineSpec, seed: int, offset: int, k: int, r: int) -> Tuple[np.ndarray, np.ndarray]:
    """``nb_synth_spline_ctrl_f32`` in float64: (ctrl [P, 3] float64 rows (X, Y, r_eff), stroke_off [k + 1] int32)."""
    counts = synth_counts_numpy(spec, seed, offset, k)
    off = np.zeros(int(k) + 1, np.int32)
    np.cumsum(counts, out=off[1:])
    radii = synth_radii_numpy(spec, seed, offset, k)
    s = _samples(offset, k)
    ctrl = np.zeros((int(off[-1]), 3), np.float64)
    fr = float(r)
    for d in range(int(k)):
        n = int(counts[d])
        t = _draw(np.arange(CTRL_DRAW0, CTRL_DRAW0 + n, dtype=np.uint64), s[d], seed)
        ux, uy = _unit(t[1]), _unit(t[2])
        if spec.mode == "cells":
            x, y = (ux * F1_1 - F0_05) * fr, (uy * F1_1 - F0_05) * fr
            free = list(range(16))
            for i in range(min(n, 16)):
                cell = free.pop(int(t[0][i]) % (16 - i))
                x[i], y[i] = (cell % 4 + ux[i]) * (fr / 4), (cell // 4 + uy[i]) * (fr / 4)
        else:
            x, y = (ux * F1_1) * fr, (uy * F1_1) * fr
        rows = ctrl[off[d]:off[d + 1]]
        rows[:, 0], rows[:, 1], rows[:, 2] = x, y, radii[d] if radii[d] >= 2 else 0.5
    return ctrl, off


def segment_offsets(stroke_off: np.ndarray, subdiv: int = SUBDIV) -> np.ndarray:
    """[k + 1] int32: the first segment row of every one-stroke drawing, ``(stroke_off[s] - 3 s) * subdiv`` (nb_spline_flatten_f32)."""
    off = np.asarray(stroke_off, np.int64)
    return ((off - 3 * np.arange(off.shape[0])) * int(subdiv)).astype(np.int32)


def raster_batch_numpy(segs: np.ndarray, seg_off: Sequence[int], out_shape: Tuple[int, int], offset=(0, 0)) -> np.ndarray:
    """``nb_raster_batch_u8`` over ``strokes.raster_segments_numpy``: [k, h, w] uint8, drawing i from rows seg_off[i] .. seg_off[i + 1];
    a range outside the rows, or a decreasing one, is empty."""
    segs = np.asarray(segs)
    out = np.full((len(seg_off) - 1, int(out_shape[0]), int(out_shape[1])), 255, np.uint8)
    for i in range(out.shape[0]):
        a, b = int(seg_off[i]), int(seg_off[i + 1])
        if 0 <= a <= b <= segs.shape[0]:
            raster_segments_numpy(segs[a:b], out.shape[1:], offset, out[i])
    return out


def _stream(device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


class SplineSynth:
    """Seeded synthetic drawings of side ``r``.  Drawing ``i`` is a function of (spec, r, seed, i) alone: ``batch(k, offset)`` gives
    drawings offset .. offset + k - 1 at any batch size.  On a CUDA/HIP device everything is enqueued on the current stream and nothing
    is read back; on a CPU device the numpy statements run (float64 on the float32 control points)."""

    def __init__(self, spec: Optional[SplineSpec] = None, r: int = REFERENCE_WIDTH, seed: int = 0, device="cpu", subdiv: int = SUBDIV):
        self.spec = spec if spec is not None else SplineSpec().scaled(r)
        self.r, self.seed, self.device, self.subdiv = int(r), int(seed) & MASK64, torch.device(device), int(subdiv)
        if self.r < 1:
            raise ValueError(f"SplineSynth: side {r}")

    @property
    def on_device(self) -> bool:
        return self.device.type == "cuda"

    def counts(self, k: int, offset: int = 0, spec: Optional[SplineSpec] = None) -> np.ndarray:
        """[k] int32 on the host (``nb_synth_spline_counts``: no HIP call)."""
        out = np.zeros(int(k), np.int32)
        c = (spec or self.spec).to_c()
        _lib.check(_lib.lib().nb_synth_spline_counts(ctypes.addressof(c), self.seed, int(offset) & MASK64, int(k), out.ctypes.data),
                   "synth_spline_counts")
        return out

    def control(self, k: int, offset: int = 0, spec: Optional[SplineSpec] = None) -> Tuple[torch.Tensor, np.ndarray]:
        """(ctrl [P, 3] float32 on the device, stroke_off [k + 1] int32 on the host) of drawings offset .. offset + k - 1."""
        spec = spec or self.spec
        if int(k) < 1:
            raise ValueError(f"SplineSynth: {k} drawings")
        if not self.on_device:
            ctrl, off = synth_ctrl_numpy(spec, self.seed, offset, k, self.r)
            return torch.from_numpy(ctrl.astype(np.float32)), off
        off = np.zeros(int(k) + 1, np.int32)
        np.cumsum(self.counts(k, offset, spec), out=off[1:])
        d_off = torch.from_numpy(off).to(self.device, non_blocking=True)
        ctrl = torch.empty([int(off[-1]), 3], dtype=torch.float32, device=self.device)
        c = spec.to_c()
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().nb_synth_spline_ctrl_f32(ctypes.addressof(c), self.seed, int(offset) & MASK64, int(k), self.r,
                                                           d_off.data_ptr(), ctrl.data_ptr(), int(off[-1]), _stream(self.device)),
                       "synth_spline_ctrl")
        return ctrl, off

    def segments(self, k: int, offset: int = 0, spec: Optional[SplineSpec] = None) -> Tuple[torch.Tensor, np.ndarray]:
        """(segs [n, SEG_PITCH] float32, seg_off [k + 1] int32 on the host): the flattened rows of the k drawings."""
        ctrl, off = self.control(k, offset, spec)
        seg_off = segment_offsets(off, self.subdiv)
        n = int(seg_off[-1])
        if not self.on_device:
            segs = np.zeros((n, SEG_PITCH), np.float32)
            segs[:, :5] = flatten_splines_numpy(ctrl.numpy(), off, self.subdiv)
            return torch.from_numpy(segs), seg_off
        segs = torch.empty([n, SEG_PITCH], dtype=torch.float32, device=self.device)
        d_off = torch.from_numpy(off).to(self.device, non_blocking=True)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().nb_spline_flatten_f32(ctrl.data_ptr(), d_off.data_ptr(), ctrl.shape[0], int(k), self.subdiv, 0.5,
                                                        segs.data_ptr(), n, _stream(self.device)), "spline_flatten")
        return segs, seg_off

    def batch(self, k: int, offset: int = 0, spec: Optional[SplineSpec] = None) -> torch.Tensor:
        """[k, r, r] uint8 on the device, 255 = background, 0 = stroke."""
        segs, seg_off = self.segments(k, offset, spec)
        return raster_batch(segs, seg_off, (self.r, self.r), device=self.device)

    def strokes(self, i: int, spec: Optional[SplineSpec] = None) -> StrokeList:
        """Drawing ``i`` as a one-spline ``StrokeList`` (``through_ends=False``: the control points are the spline's own), from the
        float32 control points the raster used: to be painted as vector strokes or saved as JSON."""
        ctrl, _ = self.control(1, int(i), spec)
        c = ctrl.cpu().numpy()
        return StrokeList().add_spline(c[:, :2], c[:, 2], through_ends=False)

    def pairs(self, k: int, radii=(16, 25), offset: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
        """(medium, thick) [k, r, r] uint8: the same k curves at two fixed radii in pixels -- the calibration set of the UVS mapper
        (the reference's ``*_rad016.png`` / ``*_rad025.png`` pairs, ``--use_radii 16 25``).  The curve does not depend on the thickness."""
        medium, thick = (self.batch(k, offset, self.spec.fixed(rad)) for rad in radii)
        return medium, thick


def raster_batch(segs: torch.Tensor, seg_off, out_shape, offset=(0, 0), device=None) -> torch.Tensor:
    """``nb_raster_batch_u8`` on device rows [n, SEG_PITCH] (``raster_batch_numpy`` for host tensors): [k, h, w] uint8.  ``seg_off``
    [k + 1]: a host array (uploaded) or a device int32 tensor."""
    device = torch.device(device) if device is not None else segs.device
    h, w = int(out_shape[0]), int(out_shape[1])
    if device.type != "cuda":
        return torch.from_numpy(raster_batch_numpy(segs.numpy(), np.asarray(seg_off), (h, w), offset))
    if segs.dtype != torch.float32 or segs.dim() != 2 or segs.shape[1] != SEG_PITCH or not segs.is_contiguous():
        raise ValueError(f"raster_batch: contiguous float32 [n, {SEG_PITCH}] expected, got {segs.dtype} {tuple(segs.shape)}")
    d_off = seg_off if isinstance(seg_off, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(seg_off, np.int32)).to(device, non_blocking=True)
    k = d_off.shape[0] - 1
    out = torch.empty([k, h, w], dtype=torch.uint8, device=device)
    with torch.cuda.device(device):
        _lib.check(_lib.lib().nb_raster_batch_u8(segs.data_ptr() if segs.shape[0] else None, d_off.data_ptr(), segs.shape[0], k, out.data_ptr(),
                                                 h, w, int(offset[0]), int(offset[1]), _stream(device)), "raster_batch")
    return out


# ---------------------------------------------------------------------------------------------------------------------
# loaders: a file of drawings, or ``synth:...``
# ---------------------------------------------------------------------------------------------------------------------
SYNTH_KEYS = ("mode", "pts", "radii", "thick", "size")


def is_synth(arg) -> bool:
    return isinstance(arg, str) and (arg == "synth" or arg.startswith("synth:"))


def _int(text: str, what: str) -> int:
    try:
        return int(text, 0)
    except ValueError:
        raise ValueError(f"synthetic drawings: {what} {text!r} is not an integer") from None


def _span(text: str, key: str) -> Tuple[int, int]:
    lo, sep, hi = text.partition("-")
    if not sep:
        raise ValueError(f"synthetic drawings: {key}={text!r}: MIN-MAX expected")
    return _int(lo, key), _int(hi, key)


def parse_synth(arg: str, r: int):
    """``synth:K[:seed[:key=value,...]]`` -> (K, seed, spec, radii or None, size).  Keys: ``mode=cells|uniform``; ``pts=MIN-MAX``;
    ``radii=A[/B...]`` fixed radii in pixels, drawing k taking radii[k mod n]; ``thick=gauss|rand|MIN-MAX`` (the reference's two
    distributions scaled by r / 256, or an integer range in pixels); ``size=D`` drawings of side D > r (full-size drawings of the
    stitching scores; thickness stays that of r-pixel patches).  ValueError names the part that is wrong."""
    parts = arg.split(":", 3)
    if parts[0] != "synth" or len(parts) < 2 or not parts[1]:
        raise ValueError(f"synthetic drawings: {arg!r}: synth:K[:seed[:key=value,...]] expected")
    k = _int(parts[1], "K")
    if k < 1:
        raise ValueError(f"synthetic drawings: K {k} must be at least 1")
    seed = _int(parts[2], "seed") if len(parts) > 2 and parts[2] else 0
    kw, radii, size, px_range = {}, None, int(r), None
    for item in (parts[3].split(",") if len(parts) > 3 and parts[3] else []):
        key, sep, val = item.partition("=")
        if key not in SYNTH_KEYS or not sep or not val:
            raise ValueError(f"synthetic drawings: unknown or empty key {key!r} in {item!r} (keys: {', '.join(SYNTH_KEYS)})")
        if key == "mode":
            if val not in _lib.NB_SPLINE_MODES:
                raise ValueError(f"synthetic drawings: mode={val!r} is none of {sorted(_lib.NB_SPLINE_MODES)}")
            kw["mode"] = val
        elif key == "pts":
            kw["pts_min"], kw["pts_max"] = _span(val, "pts")
        elif key == "radii":
            radii = [_int(v, "radii") for v in val.split("/")]
            if min(radii) < 0:
                raise ValueError(f"synthetic drawings: radii={val!r} holds a negative radius")
        elif key == "thick":
            if val == "gauss":
                kw["thick"] = "mixture"
            elif val == "rand":
                kw["thick"] = "range"
            else:
                kw["thick"], px_range = "range", _span(val, "thick")
        elif key == "size":
            size = _int(val, "size")
            if size <= int(r):
                raise ValueError(f"synthetic drawings: size={size} must exceed the patch width {r}")
    try:
        spec = dataclasses.replace(SplineSpec(), **kw).scaled(r)
        if px_range is not None:                                   # given in pixels: not scaled
            spec = dataclasses.replace(spec, rmin=px_range[0], rmax=px_range[1])
    except ValueError as e:
        raise ValueError(f"synthetic drawings: {arg!r}: {e}") from None
    return k, seed, spec, radii, size


def read_drawings(path: str) -> np.ndarray:
    """The .npz reader of the brush tools: the ``drawings`` array, or the file's first, as uint8."""
    with np.load(path) as z:
        return np.asarray(z["drawings"] if "drawings" in z.files else z[z.files[0]], np.uint8)


def load_drawings(arg: str, r: Optional[int] = None, device="cpu") -> np.ndarray:
    """[K, D, D] uint8 on the host, 0 = stroke: the .npz at ``arg``, or K synthetic drawings for ``synth:K[:seed[:key=value,...]]``
    (``parse_synth``) of side ``r`` (``size=D``: D), made on ``device``."""
    if not is_synth(arg):
        return read_drawings(arg)
    if r is None:
        raise ValueError("synthetic drawings need the patch width")
    k, seed, spec, radii, size = parse_synth(arg, int(r))
    synth = SplineSynth(spec, size, seed, device)
    if radii is None:
        return synth.batch(k).cpu().numpy()
    sets = [synth.batch(k, 0, spec.fixed(rad)).cpu().numpy() for rad in radii]
    return np.stack([sets[i % len(radii)][i] for i in range(k)])


def load_calibration(arg: str, r: Optional[int] = None, device="cpu", min_background: int = MIN_BACKGROUND) -> Tuple[np.ndarray, np.ndarray]:
    """(medium, thick) uint8 calibration drawings of ``StyleUVSMapper``: the two arrays of the .npz at ``arg``, or, for
    ``synth[:seed]``, five seeded curves in cells at the reference's two radii (16 and 25 of 256 pixels, scaled to ``r``).  A curve
    whose thick drawing leaves fewer than ``min_background`` (15) background pixels is replaced by the one at the next unused offset, at most
    ``CALIBRATION_RETRIES`` times in all."""
    if not is_synth(arg):
        with np.load(arg) as z:
            return z["medium"], z["thick"]
    if r is None:
        raise ValueError("synthetic drawings need the patch width")
    parts = arg.split(":")
    if len(parts) > 2:
        raise ValueError(f"synthetic calibration: {arg!r}: synth[:seed] expected")
    seed = _int(parts[1], "seed") if len(parts) == 2 and parts[1] else 0
    radii = [max(int(np.rint(rad * int(r) / REFERENCE_WIDTH)), 1) for rad in CALIBRATION_RADII]
    synth = SplineSynth(SplineSpec(mode="cells").scaled(r), int(r), seed, device)
    medium, thick = (t.cpu().numpy() for t in synth.pairs(CALIBRATION_K, radii))
    nxt = CALIBRATION_K
    for i in range(CALIBRATION_K):
        while int((thick[i] == 255).sum()) < min_background:
            if nxt >= CALIBRATION_K + CALIBRATION_RETRIES:
                raise RuntimeError(f"synthetic calibration: no curve with {min_background} background pixels at radius {radii[1]} in "
                                   f"{CALIBRATION_RETRIES} further draws (seed {seed}, side {r})")
            m, t = synth.pairs(1, radii, offset=nxt)
            medium[i], thick[i] = m[0].cpu().numpy(), t[0].cpu().numpy()
            nxt += 1
    return medium, thick


def save_pngs(png_dir: str, drawings: np.ndarray, radius_of, per: int = 1, first: int = 0) -> List[str]:
    """``spline%06d_rad%03d.png`` per drawing, the reference's names (create_splines.py:61); ``per`` consecutive drawings are one
    curve at several radii and share its number."""
    from PIL import Image
    os.makedirs(png_dir, exist_ok=True)
    paths = []
    for i, img in enumerate(drawings):
        paths.append(os.path.join(png_dir, "spline%06d_rad%03d.png" % (first + i // per, int(radius_of(i)))))
        Image.fromarray(np.asarray(img, np.uint8)).save(paths[-1])
    return paths
