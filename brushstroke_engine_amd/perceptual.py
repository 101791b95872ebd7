"""The LPIPS network on the device: the perceptual item of brush projection (``scripts/project_main.py:158``) and of the clarity
optimisation (``scripts/opt_clarity_main.py:282``).  The reference calls the ``lpips`` package; this module states the network itself
and loads the two small weight files a user has (``tools/convert_lpips_weights.py`` writes them into one ``.npz``).  No weights ship.

For images ``x0`` (target) and ``x1`` in -1..1, ``[N,3,H,W]``:

* scaling ``(x - shift_c) / scale_c``;
* the trunk -- torchvision's ``vgg16.features`` or ``alexnet.features`` -- with five taps at ReLU outputs;
* the head, per level and pixel: ``u = f / (sqrt(sum_c f_c^2) + 1e-10)`` for both images, ``d = sum_c w_c (u0_c - u1_c)^2``, and the
  result ``[N]`` is the sum over the levels of the spatial mean of ``d``.  ``w`` is the level's 1x1 convolution, of any sign.

Stated departure from the package: where a pixel's feature vector is all zero, the gradient through its norm is ZERO (the package's
``sqrt`` gives NaN there), and so is the rest of that pixel's gradient (which the 1e-10 would scale by 1e10).  Both routes follow
this convention.

Channel counts come from the weight arrays, so slim networks of the same layer layout run too.

``route="hip"``: the trunk's convolutions run through ``ops.conv2d`` (forward) and its input gradient, whichever kernel they pick;
everything else -- scaling, bias + ReLU + tap + pool, the head, and their backward -- runs on the entries of ``csrc/nb_lpips.hip``
inside one ``torch.autograd.Function`` that returns ``[N]`` and differentiates the second image only.  ``route="torch"`` is the same
definition in float32 torch operations; it runs on the CPU and is what the tests compare against.

``LPIPS.pair_distance(x)`` serves the perceptual brush scores (``metrics``): ``x`` holds the first images of n pairs in rows ``:n`` and
the second in rows ``n:`` (what ``ops.metric_pairs`` writes), the trunk runs once over all 2n, and no gradient is kept.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import numpy as np
import torch
import torch.nn.functional as F

SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
EPS = 1e-10

# conv index -> (stride, padding); pool index -> window (stride 2, floor mode, no padding); taps = ReLU outputs
ARCHS = {
    "vgg": dict(convs={i: (1, 1) for i in (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)}, kernels={}, pools={4: 2, 9: 2, 16: 2, 23: 2},
                taps=(3, 8, 15, 22, 29)),
    "alex": dict(convs={0: (4, 2), 3: (1, 2), 6: (1, 1), 8: (1, 1), 10: (1, 1)}, kernels={0: 11, 3: 5}, pools={2: 3, 5: 3}, taps=(1, 4, 7, 9, 11)),
}


class _Layer:
    """One convolution of the trunk with what follows it: ReLU (index + 1), perhaps a tap, perhaps a pool (index + 2)."""

    def __init__(self, index, stride, padding, level, window):
        self.index, self.stride, self.padding, self.level, self.window = index, stride, padding, level, window


def layer_plan(arch: str) -> List[_Layer]:
    a = ARCHS[arch]
    return [_Layer(i, s, p, a["taps"].index(i + 1) if i + 1 in a["taps"] else None, a["pools"].get(i + 2, 0)) for i, (s, p) in sorted(a["convs"].items())]


def _sizes_ok(arch: str, side: int) -> bool:
    """Whether an image of ``side`` pixels passes every convolution and pool of the trunk with at least one output pixel."""
    kernels = ARCHS[arch]["kernels"]
    for lay in layer_plan(arch):
        side = (side + 2 * lay.padding - kernels.get(lay.index, 3)) // lay.stride + 1
        if side < 1 or (lay.window and side < lay.window):
            return False
        if lay.window:
            side = (side - lay.window) // 2 + 1
    return True


def min_size(arch: str) -> int:
    """The smallest image side the trunk of ``arch`` accepts, from ``ARCHS`` (alex 31, vgg 16): below it a pool has no window."""
    return next(s for s in range(1, 1 << 12) if _sizes_ok(arch, s))


def unit(f: torch.Tensor) -> torch.Tensor:
    """f / (sqrt(sum_c f_c^2) + 1e-10) over the channels; a pixel whose vector is all zero gives zeros and takes no gradient."""
    ss = f.square().sum(dim=1, keepdim=True)
    pos = ss > 0
    return torch.where(pos, f / (torch.where(pos, ss, torch.ones_like(ss)).sqrt() + EPS), torch.zeros_like(f))


def head_torch(f0: torch.Tensor, f1: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """[N]: mean over pixels of sum_c w_c (u0_c - u1_c)^2 of one level."""
    u0, u1 = unit(f0), unit(f1)
    return ((u0 - u1).square() * w.reshape(1, -1, 1, 1)).sum(dim=1).mean(dim=(1, 2))


def _stream():
    return torch.cuda.current_stream().cuda_stream


class _HipKernels:
    """The entries of csrc/nb_lpips.hip on dense float32 tensors."""

    @staticmethod
    def scale(x, shift, scale):
        from . import _lib
        x = x.contiguous()
        n, c = x.shape[0], x.shape[1]
        y = torch.empty_like(x)
        with torch.cuda.device(x.device):
            _lib.check(_lib.lib().nb_lpips_scale_f32(x.data_ptr(), None if shift is None else shift.data_ptr(), scale.data_ptr(), y.data_ptr(), n, c,
                                                     x.shape[2] * x.shape[3], _stream()), "lpips_scale")
        return y

    @staticmethod
    def relu_pool(x, bias, window):
        from . import _lib
        x = x.contiguous()
        n, c, h, w = x.shape
        tap = torch.empty_like(x)
        pooled = torch.empty([n, c, (h - window) // 2 + 1, (w - window) // 2 + 1], dtype=torch.float32, device=x.device) if window else None
        with torch.cuda.device(x.device):
            _lib.check(_lib.lib().nb_lpips_relu_pool_f32(x.data_ptr(), bias.data_ptr(), tap.data_ptr(), None if pooled is None else pooled.data_ptr(),
                                                         n, c, h, w, window, _stream()), "lpips_relu_pool")
        return tap, pooled

    @staticmethod
    def relu_pool_bwd(tap, d_tap, d_pooled, window):
        from . import _lib
        n, c, h, w = tap.shape
        d_tap = None if d_tap is None else d_tap.contiguous()
        d_pooled = None if d_pooled is None else d_pooled.contiguous()
        d_x = torch.empty_like(tap)
        with torch.cuda.device(tap.device):
            _lib.check(_lib.lib().nb_lpips_relu_pool_bwd_f32(tap.data_ptr(), None if d_tap is None else d_tap.data_ptr(),
                                                             None if d_pooled is None else d_pooled.data_ptr(), d_x.data_ptr(), n, c, h, w, window,
                                                             _stream()), "lpips_relu_pool_bwd")
        return d_x

    @staticmethod
    def head(f0, f1, w, acc):
        """Adds the level's [N] into ``acc``; returns the kept per-pixel values [3,N,H*W]."""
        from . import _lib
        assert f0.shape == f1.shape and f0.is_contiguous() and f1.is_contiguous()
        n, c, hw = f0.shape[0], f0.shape[1], f0.shape[2] * f0.shape[3]
        parts = int(_lib.lib().nb_lpips_head_parts(c, hw))
        kept = torch.empty([3, n, hw], dtype=torch.float32, device=f0.device)
        partials = torch.empty([max(n * parts, 1)], dtype=torch.float32, device=f0.device)
        with torch.cuda.device(f0.device):
            _lib.check(_lib.lib().nb_lpips_head_f32(f0.data_ptr(), f1.data_ptr(), w.data_ptr(), n, c, hw, kept.data_ptr(), partials.data_ptr(),
                                                    acc.data_ptr(), _stream()), "lpips_head")
        return kept

    @staticmethod
    def head_bwd(f0, f1, w, kept, g, out=None):
        """d_f1; added into ``out`` when it is given."""
        from . import _lib
        n, c, hw = f0.shape[0], f0.shape[1], f0.shape[2] * f0.shape[3]
        d = torch.empty_like(f1) if out is None else out
        assert d.is_contiguous()
        with torch.cuda.device(f0.device):
            _lib.check(_lib.lib().nb_lpips_head_bwd_f32(f0.data_ptr(), f1.data_ptr(), w.data_ptr(), kept.data_ptr(), g.data_ptr(), n, c, hw,
                                                        int(out is not None), d.data_ptr(), _stream()), "lpips_head_bwd")
        return d


def _conv_input_grad(d_raw, net, lay, x_shape):
    """Gradient of a trunk convolution's input.  Stride 1: ``ops.conv2d``'s own input gradient.  The strided first layer of ``alex``
    (11x11, stride 4, padding 2): zero-stuffing, then a stride-1 correlation with the transposed, flipped kernel (kept from
    construction) through ``ops.conv2d``, the stuffed gradient padded on the right and below so that the rows and columns which only
    the LAST window reaches are computed (64 = 4 * 14 + 11 - 2 * 2 + 1: one column more than a symmetric padding of 8 yields)."""
    from . import ops
    w = net.weights[lay.index]
    if lay.stride == 1:
        return ops._conv2d_input_grad(d_raw, w, x_shape, 1, lay.padding)
    k, s, p = w.shape[2], lay.stride, lay.padding
    dy = ops.upfirdn2d(d_raw, None, up=s, padding=[0, -(s - 1), 0, -(s - 1)])
    eh, ew = (x_shape[2] - ((d_raw.shape[2] - 1) * s + k - 2 * p)), (x_shape[3] - ((d_raw.shape[3] - 1) * s + k - 2 * p))
    dy = F.pad(dy, (0, ew, 0, eh))
    return ops.conv2d(dy, net.weights_tf[lay.index], stride=1, padding=k - 1 - p)


class _LpipsHip(torch.autograd.Function):
    """[N] = LPIPS(target, x1) on the kernels, for target taps already computed; differentiates ``x1``."""

    @staticmethod
    def forward(ctx, x1, net, taps0):
        from . import ops
        K = _HipKernels
        x = K.scale(x1.detach().to(torch.float32), net.shift, net.scale)
        acc = torch.zeros([x.shape[0]], dtype=torch.float32, device=x.device)
        shapes, taps, kept = [], [], {}
        net.trunk_calls += 1
        for lay in net.plan:
            shapes.append(tuple(x.shape))
            raw = ops.conv2d(x, net.weights[lay.index], stride=lay.stride, padding=lay.padding)
            tap, pooled = K.relu_pool(raw, net.biases[lay.index], lay.window)
            del raw
            taps.append(tap)
            if lay.level is not None:
                kept[lay.level] = K.head(taps0[lay.level], tap, net.lins[lay.level], acc)
            x = pooled if lay.window else tap
        ctx.net, ctx.taps0, ctx.shapes, ctx.taps, ctx.kept = net, taps0, shapes, taps, kept
        return acc

    @staticmethod
    def backward(ctx, g):
        K, net = _HipKernels, ctx.net
        g = g.detach().to(torch.float32).contiguous()
        d_next = None                                                      # gradient of what the layer hands to the next convolution
        with torch.no_grad():
            for j in range(len(net.plan) - 1, -1, -1):
                lay, tap = net.plan[j], ctx.taps[j]
                d_tap, d_pooled = (None, d_next) if lay.window else (d_next, None)
                if lay.level is not None:
                    d_tap = K.head_bwd(ctx.taps0[lay.level], tap, net.lins[lay.level], ctx.kept[lay.level], g,
                                       out=None if d_tap is None else d_tap.contiguous())
                d_raw = K.relu_pool_bwd(tap, d_tap, d_pooled, lay.window)
                d_next = _conv_input_grad(d_raw, net, lay, ctx.shapes[j])
            d_x1 = K.scale(d_next, None, net.scale)
        return d_x1, None, None


class LPIPS:
    """``LPIPS(weights)(target, synth) -> [N]``.

    ``weights``: the path of a ``.npz`` or a dict of arrays with ``features.<i>.weight`` / ``features.<i>.bias`` under torchvision's
    indices, ``lin<l>.weight`` ``[C_l]`` for the five levels, ``arch`` (``"vgg"`` or ``"alex"``; ``net`` overrides it) and optionally
    ``scaling.shift`` / ``scaling.scale``.  ``route``: ``"hip"`` (the default on a GPU; there is no CPU fallback) or ``"torch"``.
    The weights are constants: they are converted and placed on the device once, here, and the module takes no gradient for them.

    A zero-norm pixel of a feature map passes no gradient through its norm (module docstring)."""

    def __init__(self, weights, net: Optional[str] = None, route: Optional[str] = None, device=None):
        if isinstance(weights, (str, bytes)) or hasattr(weights, "__fspath__"):
            with np.load(weights, allow_pickle=False) as z:
                weights = {k: z[k] for k in z.files}
        arch = net if net is not None else (str(np.asarray(weights["arch"]).reshape(-1)[0]) if "arch" in weights else None)
        if arch not in ARCHS:
            raise ValueError(f"LPIPS: arch {arch!r}: 'vgg' or 'alex' (the weights' 'arch' entry or the net argument)")
        self.arch, self.plan = arch, layer_plan(arch)
        self.device = torch.device(device if device is not None else ("cuda" if torch.cuda.is_available() else "cpu"))
        self.route = route if route is not None else ("hip" if self.device.type == "cuda" else "torch")
        if self.route not in ("hip", "torch"):
            raise ValueError(f"route {self.route!r}: 'hip' or 'torch'")
        if self.route == "hip" and self.device.type != "cuda":
            from ._lib import NeubeHipError
            raise NeubeHipError("route='hip' needs a GPU (there is no CPU fallback for the LPIPS kernels)")
        t = lambda a: torch.as_tensor(np.asarray(a, np.float32)).to(self.device).contiguous()
        self.weights: Dict[int, torch.Tensor] = {}
        self.biases: Dict[int, torch.Tensor] = {}
        self.weights_tf: Dict[int, torch.Tensor] = {}
        c_in = 3
        for lay in self.plan:
            for suffix in ("weight", "bias"):
                if f"features.{lay.index}.{suffix}" not in weights:
                    raise KeyError(f"LPIPS ({arch}): the weights lack features.{lay.index}.{suffix}")
            w, b = t(weights[f"features.{lay.index}.weight"]), t(weights[f"features.{lay.index}.bias"])
            k = ARCHS[arch]["kernels"].get(lay.index, 3)
            if w.ndim != 4 or tuple(w.shape[1:]) != (c_in, k, k) or tuple(b.shape) != (w.shape[0],):
                raise ValueError(f"LPIPS ({arch}): features.{lay.index}.weight {tuple(w.shape)} / bias {tuple(b.shape)}: [C,{c_in},{k},{k}] and [C] expected")
            self.weights[lay.index], self.biases[lay.index], c_in = w, b, w.shape[0]
            if lay.stride != 1:                                            # the backward's kernel of a strided layer, once
                self.weights_tf[lay.index] = w.transpose(0, 1).flip([2, 3]).contiguous()
        self.lins: List[torch.Tensor] = []
        for lay in (l for l in self.plan if l.level is not None):
            lin = t(weights[f"lin{lay.level}.weight"]).reshape(-1)
            if lin.numel() != self.weights[lay.index].shape[0]:
                raise ValueError(f"LPIPS ({arch}): lin{lay.level}.weight has {lin.numel()} entries, the tap {self.weights[lay.index].shape[0]} channels")
            self.lins.append(lin)
        self.shift, self.scale = t(weights.get("scaling.shift", SHIFT)).reshape(3), t(weights.get("scaling.scale", SCALE)).reshape(3)
        self.trunk_calls = 0                                               # trunk passes so far (a bound target costs one per pass, not per step)

    # -- route "torch" --
    def _taps_torch(self, x: torch.Tensor) -> List[torch.Tensor]:
        self.trunk_calls += 1
        x = (x.to(torch.float32) - self.shift.reshape(1, 3, 1, 1)) / self.scale.reshape(1, 3, 1, 1)
        taps = []
        for lay in self.plan:
            x = F.relu(F.conv2d(x, self.weights[lay.index], self.biases[lay.index], stride=lay.stride, padding=lay.padding))
            if lay.level is not None:
                taps.append(x)
            if lay.window:
                x = F.max_pool2d(x, lay.window, 2)
        return taps

    # -- route "hip" --
    def _taps_hip(self, x: torch.Tensor) -> List[torch.Tensor]:
        from . import ops
        self.trunk_calls += 1
        taps = []
        with torch.no_grad():
            x = _HipKernels.scale(x.detach().to(torch.float32), self.shift, self.scale)
            for lay in self.plan:
                raw = ops.conv2d(x, self.weights[lay.index], stride=lay.stride, padding=lay.padding)
                tap, pooled = _HipKernels.relu_pool(raw, self.biases[lay.index], lay.window)
                if lay.level is not None:
                    taps.append(tap)
                x = pooled if lay.window else tap
        return taps

    def _check(self, target, synth):
        if target.ndim != 4 or target.shape[1] != 3 or (synth is not None and synth.shape != target.shape):
            raise ValueError(f"LPIPS: images [N,3,H,W] of one shape expected, got {tuple(target.shape)}" + ("" if synth is None else f" and {tuple(synth.shape)}"))

    def target_taps(self, target: torch.Tensor) -> List[torch.Tensor]:
        """The five tap maps of a target, detached: what :meth:`bind` keeps."""
        self._check(target, None)
        target = target.detach().to(self.device)
        if self.route == "hip":
            return self._taps_hip(target)
        with torch.no_grad():
            return self._taps_torch(target)

    def _with_taps(self, taps0, synth):
        synth = synth.to(self.device)
        if self.route == "hip":
            return _LpipsHip.apply(synth, self, taps0)
        out = 0
        for f0, f1, w in zip(taps0, self._taps_torch(synth), self.lins):
            out = out + head_torch(f0, f1, w)
        return out

    def __call__(self, target: torch.Tensor, synth: torch.Tensor) -> torch.Tensor:
        """[N]; differentiable with respect to ``synth`` (the target is a constant)."""
        self._check(target, synth)
        return self._with_taps(self.target_taps(target), synth)

    def pair_distance(self, x: torch.Tensor) -> torch.Tensor:
        """[n] for ``x`` [2n,3,H,W] in -1..1: LPIPS(x[i], x[n + i]), without a gradient.  ONE trunk pass over all 2n images (the batch
        that ``ops.metric_pairs`` writes, no concatenation); per level the head runs between ``tap[:n]`` and ``tap[n:]``."""
        if x.ndim != 4 or x.shape[1] != 3 or x.shape[0] % 2:
            raise ValueError(f"LPIPS.pair_distance: images [2n,3,H,W] expected, got {tuple(x.shape)}")
        need = min_size(self.arch)
        if min(x.shape[2], x.shape[3]) < need:
            raise ValueError(f"LPIPS.pair_distance ({self.arch}): images of {x.shape[2]} x {x.shape[3]} are below the trunk's minimum side {need}")
        n = x.shape[0] // 2
        x = x.detach().to(self.device)
        with torch.no_grad():
            if self.route == "hip":
                acc = torch.zeros([n], dtype=torch.float32, device=self.device)
                if n:
                    for tap, w in zip(self._taps_hip(x), self.lins):       # (tap[:n], tap[n:]: dense halves of a dense tensor)
                        _HipKernels.head(tap[:n], tap[n:], w, acc)
                return acc
            out = torch.zeros([n], dtype=torch.float32, device=self.device)
            for tap, w in zip(self._taps_torch(x), self.lins):
                out = out + head_torch(tap[:n], tap[n:], w)
            return out

    def bind(self, target: torch.Tensor):
        """A callable ``(target, synth) -> [N]`` for a FIXED target: its scaled image goes through the trunk once, here, and the five tap
        maps are kept; every call then costs one trunk pass (the synthesised image's) instead of two.  The ``target`` argument of the
        returned callable is only checked for its shape."""
        taps0, shape = self.target_taps(target), tuple(target.shape)

        def bound(target_, synth):
            if tuple(target_.shape) != shape:
                raise ValueError(f"LPIPS.bind: bound to a target of shape {shape}, called with {tuple(target_.shape)}")
            self._check(target_, synth)
            return self._with_taps(taps0, synth)

        return bound


def convert_state_dicts(trunk_sd: Dict, head_sd: Dict, arch: str) -> Dict[str, np.ndarray]:
    """The ``.npz`` entries from torchvision's state dict (``features.N.weight`` / ``.bias``) and the package's head file
    (``lin<l>.model.1.weight`` ``[1,C,1,1]``); what ``tools/convert_lpips_weights.py`` writes."""
    if arch not in ARCHS:
        raise ValueError(f"arch {arch!r}: 'vgg' or 'alex'")
    arr = lambda v: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)).astype(np.float32)
    out = {"arch": np.asarray(arch)}
    for lay in layer_plan(arch):
        for suffix in ("weight", "bias"):
            key = f"features.{lay.index}.{suffix}"
            if key not in trunk_sd:
                raise KeyError(f"the trunk's state dict lacks {key}")
            out[key] = arr(trunk_sd[key])
        if lay.level is not None:
            key = f"lin{lay.level}.model.1.weight"
            if key not in head_sd:
                raise KeyError(f"the head's state dict lacks {key}")
            lin = arr(head_sd[key])
            if lin.ndim != 4 or lin.shape[0] != 1 or lin.shape[2:] != (1, 1) or lin.shape[1] != out[f"features.{lay.index}.weight"].shape[0]:
                raise ValueError(f"{key}: shape {lin.shape}, [1,{out[f'features.{lay.index}.weight'].shape[0]},1,1] expected")
            out[f"lin{lay.level}.weight"] = lin.reshape(-1)
    out["scaling.shift"], out["scaling.scale"] = np.asarray(SHIFT, np.float32), np.asarray(SCALE, np.float32)
    return out
