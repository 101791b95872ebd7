"""Clarity optimisation of brushes: the step that PRODUCES projected brushes (W+ plus noise planes) whose background is clear --
the reference's ``scripts/opt_clarity_main.py`` -- for K brushes at once.

A brush whose ``BG_CLARITY_MEAN`` (:mod:`metrics`) is low is optimised in W+ and in the generator's noise planes against
``0.5*iou_inv(uvs)+0.5*iou(u)+50*l1(fake_orig)`` (the reference's default without its perceptual item, which needs the LPIPS network)
plus the multi-scale noise regulariser (``opt_clarity_main.py:127-137``); the result is what ``formats.WBrushLibrary`` reads.

The state of K brushes is one arena ``[K, P]`` (:class:`ArenaLayout`: W+ followed by the noise planes in ``cfg.layers`` order).  The
generator is differentiated by :class:`training.TrainableGenerator` (HIP modconv / bias-act / FIR kernels, forward and backward);
everything around it runs, with ``route="hip"``, on the four entries of ``csrc/nb_clarity.hip`` -- the fused loss and its gradient,
the regulariser's value and gradient, Adam with the per-plane renormalisation -- and with ``route="torch"`` as the reference's
operations in float32 torch (what CPU tests run and what the GPU tests and ``tools/bench_clarity.py`` compare against).
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Callable, Dict, List, Optional, Sequence

import numpy as np
import torch
import torch.nn.functional as F

from .forger_losses import ForgerLosses

DEFAULT_LOSSES = "0.5*iou_inv(uvs)+0.5*iou(u)+50*l1(fake_orig)"
_FUSED_ITEMS = ("iou_inv_uvs", "iou_u", "l1_fake_orig")
_LPIPS_ITEM = "lpips_fake_orig"
ADAM_BETAS, ADAM_EPS = (0.9, 0.999), 1e-8


# ------------------------------------------------------------------------------------------------
# host functions
# ------------------------------------------------------------------------------------------------
def w_stats(mapping: Callable, z_dim: int, num_samples: int = 10000, device="cpu"):
    """``get_w_stats`` (experiment/util/latent.py:15-32): ``RandomState(123)`` latents through ``mapping``, the first W only;
    returns (w_avg [1,1,C] float32, w_std) with w_std = sqrt(sum((w - w_avg)^2) / num_samples), a sum over samples AND channels."""
    z = np.random.RandomState(123).randn(num_samples, z_dim)
    with torch.no_grad():
        w = mapping(torch.from_numpy(z).to(device), None)
    w = w[:, :1, :].cpu().numpy().astype(np.float32)
    w_avg = np.mean(w, axis=0, keepdims=True)
    return w_avg, float((np.sum((w - w_avg) ** 2) / num_samples) ** 0.5)


def lr_and_noise_schedule(step: int, num_steps: int, w_std: float = 1.0, initial_learning_rate: float = 0.1, initial_noise_factor: float = 0.05,
                          lr_rampdown_length: float = 0.25, lr_rampup_length: float = 0.05, noise_ramp_length: float = 0.75):
    """(lr, w_noise_scale) of a step, ``opt_clarity_main.py:94-100``: cosine ramp-down over the last quarter, linear ramp-up over the
    first twentieth, W noise that fades quadratically over the first three quarters."""
    t = step / num_steps
    w_noise_scale = w_std * initial_noise_factor * max(0.0, 1.0 - t / noise_ramp_length) ** 2
    lr_ramp = min(1.0, (1.0 - t) / lr_rampdown_length)
    lr_ramp = 0.5 - 0.5 * np.cos(lr_ramp * np.pi)
    lr_ramp = lr_ramp * min(1.0, t / lr_rampup_length)
    return float(initial_learning_rate * lr_ramp), float(w_noise_scale)


class ArenaLayout:
    """A row of the arena: ``nw`` floats of W+ followed by square noise planes of sides ``res`` (powers of two), densely."""

    def __init__(self, nw: int, res: Sequence[int], names: Optional[Sequence[str]] = None, w_shape=None):
        self.nw, self.res = int(nw), [int(r) for r in res]
        self.names = list(names) if names is not None else [f"plane{i}" for i in range(len(self.res))]
        self.w_shape = tuple(w_shape) if w_shape is not None else (1, self.nw)
        assert len(self.names) == len(self.res) and int(np.prod(self.w_shape)) == self.nw
        self.off, o = [], self.nw
        for r in self.res:
            self.off.append(o)
            o += r * r
        self.p = o

    @staticmethod
    def from_config(cfg) -> "ArenaLayout":
        """W+ [num_ws, w_dim] and every layer's ``noise_const`` under the key ``OracleGenerator.synthesis`` and
        ``SynthesisNetwork.brush_noise()`` use (``b<res>.conv<i>.noise_const``)."""
        return ArenaLayout(cfg.num_ws * cfg.w_dim, [l.block_res for l in cfg.layers],
                           [l.name[len("synthesis."):] + ".noise_const" for l in cfg.layers], (cfg.num_ws, cfg.w_dim))

    def plane(self, arena: torch.Tensor, i: int) -> torch.Tensor:
        """[K, r, r] view of plane i."""
        r = self.res[i]
        return arena[:, self.off[i]:self.off[i] + r * r].view(arena.shape[0], r, r)

    def w(self, arena: torch.Tensor) -> torch.Tensor:
        return arena[:, :self.nw].view(arena.shape[0], *self.w_shape)

    def planes_struct(self):
        from . import _lib
        if len(self.res) > _lib.NB_CLARITY_MAX_PLANES:
            raise ValueError(f"at most {_lib.NB_CLARITY_MAX_PLANES} noise planes, got {len(self.res)}")
        s = _lib.NbClarityPlanes()
        s.n = len(self.res)
        for i, (r, o) in enumerate(zip(self.res, self.off)):
            s.res[i], s.off[i] = r, o
        return s


# ------------------------------------------------------------------------------------------------
# route "torch": the reference's operations, float32 (or whatever dtype the tensors have)
# ------------------------------------------------------------------------------------------------
def loss_torch(uvs, img, target, geom, k: int, weights):
    """[K, 4] = {iou_inv(uvs), iou(u), l1(fake_orig), weighted total} per brush: ``forger_losses.compute_iou`` in its per-sample form
    (eps 1e-8) and ``l1_loss`` with mean reduction, on samples n = brush * B + drawing; ``geom`` [B,1,R,R] is shared."""
    b = geom.shape[0]
    eps = 1e-8
    g = geom[:, 0].unsqueeze(0)                                            # [1,B,R,R], 1 = background
    t = 1 - g
    s, u = uvs[:, 2].reshape(k, b, *uvs.shape[2:]), uvs[:, 0].reshape(k, b, *uvs.shape[2:])
    inter = torch.sum(s * g, dim=(2, 3))
    iou_inv = 1.0 - (inter / (torch.sum(s + g, dim=(2, 3)) - inter + eps)).mean(dim=1)
    inter = torch.sum(u * t, dim=(2, 3))
    iou = 1.0 - (inter / (torch.sum(u + t, dim=(2, 3)) - inter + eps)).mean(dim=1)
    l1 = (img - target.detach()).abs().reshape(k, -1).mean(dim=1)
    return torch.stack([iou_inv, iou, l1, (weights[0] * iou_inv + weights[1] * iou) + weights[2] * l1], dim=1)


def noise_reg_torch(arena: torch.Tensor, layout: ArenaLayout) -> torch.Tensor:
    """[K]: the regulariser of ``opt_clarity_main.py:127-137`` of every row, planes in their order (differentiable)."""
    reg = torch.zeros([arena.shape[0]], dtype=arena.dtype, device=arena.device)
    for i in range(len(layout.res)):
        noise = layout.plane(arena, i).unsqueeze(1)
        while True:
            reg = reg + (noise * torch.roll(noise, shifts=1, dims=3)).mean(dim=(1, 2, 3)) ** 2
            reg = reg + (noise * torch.roll(noise, shifts=1, dims=2)).mean(dim=(1, 2, 3)) ** 2
            if noise.shape[2] <= 8:
                break
            noise = F.avg_pool2d(noise, kernel_size=2)
    return reg


@torch.no_grad()
def step_torch(arena, grad, m, v, layout: ArenaLayout, lr: float, t: int):
    """``torch.optim.Adam.step`` (defaults; single-tensor arithmetic) on the arena, then ``buf -= buf.mean(); buf *=
    buf.square().mean().rsqrt()`` per plane (``opt_clarity_main.py:159-167``).  In place."""
    b1, b2 = ADAM_BETAS
    m.lerp_(grad, 1 - b1)
    v.mul_(b2).addcmul_(grad, grad, value=1 - b2)
    step_size = lr / (1 - b1 ** t)
    denom = (v.sqrt() / math.sqrt(1 - b2 ** t)).add_(ADAM_EPS)
    arena.addcdiv_(m, denom, value=-step_size)
    for i in range(len(layout.res)):
        buf = layout.plane(arena, i)
        buf -= buf.mean(dim=(1, 2), keepdim=True)
        buf *= buf.square().mean(dim=(1, 2), keepdim=True).rsqrt()


# ------------------------------------------------------------------------------------------------
# route "hip": csrc/nb_clarity.hip
# ------------------------------------------------------------------------------------------------
def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dense_samples(t: torch.Tensor) -> torch.Tensor:
    """[N,3,R,R] whose three planes are dense (any sample stride): as it is when it is, else a contiguous copy."""
    r = t.shape[-1]
    return t if (t.stride(3) == 1 and t.stride(2) == r and t.stride(1) == r * r and t.stride(0) >= 3 * r * r) else t.contiguous()


class _FusedClarityLoss(torch.autograd.Function):
    """The three-item loss on ``nb_clarity_loss_f32`` / ``nb_clarity_loss_bwd_f32``: returns (total [K], items [K,3]); gradients flow
    through the totals to ``uvs`` and ``img`` (the items are reported values)."""

    @staticmethod
    def forward(ctx, uvs, img, target, geom, k, weights):
        from . import _lib
        uvs, img, target = _dense_samples(uvs.detach()), _dense_samples(img.detach()), _dense_samples(target.detach())
        geom = geom.detach().to(torch.float32).contiguous()
        b, r = geom.shape[0], geom.shape[-1]
        assert uvs.shape == (k * b, 3, r, r) and img.shape == uvs.shape and target.shape == uvs.shape and uvs.dtype == torch.float32
        dev = uvs.device
        out = torch.empty([k, 4], dtype=torch.float32, device=dev)
        sums = torch.empty([k * b, 8], dtype=torch.float32, device=dev)
        partials = torch.empty([k * b * _lib.NB_CLARITY_LOSS_PARTS * 8], dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().nb_clarity_loss_f32(uvs.data_ptr(), uvs.stride(0), img.data_ptr(), img.stride(0), target.data_ptr(), target.stride(0),
                                                      geom.data_ptr(), k, b, r, weights[0], weights[1], weights[2], out.data_ptr(), sums.data_ptr(),
                                                      partials.data_ptr(), _stream()), "clarity_loss")
        ctx.save_for_backward(img, target, geom, sums)
        ctx.k, ctx.weights = k, weights
        total, items = out[:, 3].clone(), out[:, :3].clone()
        ctx.mark_non_differentiable(items)
        return total, items

    @staticmethod
    def backward(ctx, g_total, _g_items):
        from . import _lib
        img, target, geom, sums = ctx.saved_tensors
        k, w = ctx.k, ctx.weights
        b, r = geom.shape[0], geom.shape[-1]
        gscale = g_total.to(torch.float32).contiguous()
        d_uvs, d_img = torch.empty([k * b, 3, r, r], dtype=torch.float32, device=img.device), torch.empty([k * b, 3, r, r], dtype=torch.float32, device=img.device)
        with torch.cuda.device(img.device):
            _lib.check(_lib.lib().nb_clarity_loss_bwd_f32(img.data_ptr(), img.stride(0), target.data_ptr(), target.stride(0), geom.data_ptr(),
                                                          sums.data_ptr(), gscale.data_ptr(), k, b, r, w[0], w[1], w[2], d_uvs.data_ptr(),
                                                          d_img.data_ptr(), _stream()), "clarity_loss_bwd")
        return d_uvs, d_img, None, None, None, None


def fused_clarity_loss(uvs, img, target, geom, k: int, weights):
    """(total [K], items [K,3]) on the HIP kernels; the arguments of :func:`loss_torch`."""
    return _FusedClarityLoss.apply(uvs, img, target, geom, int(k), tuple(float(x) for x in weights))


class HipArenaOps:
    """The regulariser and the step of a layout on ``nb_noise_reg_f32`` / ``nb_clarity_step_f32``, with their scratch."""

    def __init__(self, layout: ArenaLayout, k: int, device):
        from . import _lib
        self._lib, self.layout, self.k, self.device = _lib, layout, int(k), torch.device(device)
        self.planes = layout.planes_struct()
        n = _lib.lib().nb_clarity_scratch_floats(C.byref(self.planes), layout.nw, layout.p, self.k)
        if n < 0:
            _lib.check(_lib.NB_EINVAL, "clarity_scratch_floats")
        self.scratch = torch.empty([max(int(n), 1)], dtype=torch.float32, device=self.device)

    def _check_rows(self, *ts):
        for t in ts:
            assert t.dtype == torch.float32 and t.shape == (self.k, self.layout.p) and t.stride(1) == 1 and t.device == self.device

    def noise_reg(self, arena: torch.Tensor, grad: Optional[torch.Tensor], weight: float) -> torch.Tensor:
        """[K] values; the gradient is added, times ``weight``, into ``grad`` (None: the values only)."""
        self._check_rows(arena, *([grad] if grad is not None else []))
        reg = torch.empty([self.k], dtype=torch.float32, device=self.device)
        lo = self.layout
        with torch.cuda.device(self.device):
            self._lib.check(self._lib.lib().nb_noise_reg_f32(arena.data_ptr(), arena.stride(0), lo.p, lo.nw, C.byref(self.planes), self.k, float(weight),
                                                             None if grad is None else grad.data_ptr(), 0 if grad is None else grad.stride(0),
                                                             reg.data_ptr(), self.scratch.data_ptr(), self.scratch.numel(), _stream()), "noise_reg")
        return reg

    def step(self, arena, grad, m, v, lr: float, t: int):
        self._check_rows(arena, grad, m, v)
        assert arena.stride(0) == grad.stride(0) == m.stride(0) == v.stride(0)
        lo = self.layout
        with torch.cuda.device(self.device):
            self._lib.check(self._lib.lib().nb_clarity_step_f32(arena.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(), arena.stride(0), lo.p, lo.nw,
                                                                C.byref(self.planes), self.k, float(lr), int(t), self.scratch.data_ptr(),
                                                                self.scratch.numel(), _stream()), "clarity_step")


# ------------------------------------------------------------------------------------------------
# the loop
# ------------------------------------------------------------------------------------------------
class ClarityDraws:
    """The random draws of a run.  Every brush has a generator of its own (initial noise planes, the W noise of each step) and the
    drawings of step i are the same for every brush, so what a brush ends as does not depend on which brushes share its pass."""

    def __init__(self, seed: int, num_drawings: int):
        self.seed, self.num_drawings = int(seed), int(num_drawings)
        self._gens: Dict[int, torch.Generator] = {}

    def _gen(self, brush: int) -> torch.Generator:
        if brush not in self._gens:
            self._gens[brush] = torch.Generator().manual_seed((self.seed * 1000003 + 7919 * (brush + 1)) % (2 ** 63))
        return self._gens[brush]

    def drawings(self, step: int, batch_size: int) -> torch.Tensor:
        g = torch.Generator().manual_seed((self.seed * 1000003 + 15485863 * (step + 1) + 1) % (2 ** 63))
        return torch.randint(0, self.num_drawings, (batch_size,), generator=g)

    def initial_noise(self, brush: int, numel: int) -> torch.Tensor:
        return torch.randn([numel], dtype=torch.float32, generator=self._gen(brush))

    def w_noise(self, step: int, brush: int, shape) -> torch.Tensor:
        return torch.randn(list(shape), dtype=torch.float32, generator=self._gen(brush))


class ClarityOptimizer:
    """``run_one_clarity_opt`` (opt_clarity_main.py:56-169) for batches of brushes.

    ``gen``: a differentiable generator with ``cfg``, ``mapping(z, None)`` and ``synthesis(ws, geom_feature, noise_mode="const",
    noise_buffers=..., return_debug_data=True)`` -- ``training.TrainableGenerator`` on the GPU.  ``encode``: [B,1,R,R] float drawings
    (1 = background) -> the list of geometry features.  ``drawings_u8`` [N,R,R] uint8, 0 = stroke: the conditioning AND the truth
    (the reference's ``__main__`` passes ``geom_input_channel`` for both).  ``losses``: a :mod:`forger_losses` string; the three items
    of :data:`DEFAULT_LOSSES` (any weights) run fused with ``route="hip"``, any other string goes through ``ForgerLosses.compute``.
    ``lpips``: a :class:`perceptual.LPIPS` (any callable ``(target, source) -> [N]``), which allows ``lpips(<component>)`` in the
    string; the three fused items plus ``lpips(fake_orig)`` -- the reference's default -- stay on the fused kernels, with the
    perceptual term added per brush and reported as a fourth item."""

    def __init__(self, gen, encode: Callable, drawings_u8, losses: str = DEFAULT_LOSSES, regularize_noise_weight: float = 10,
                 initial_learning_rate: float = 0.1, initial_noise_factor: float = 0.05, lr_rampdown_length: float = 0.25,
                 lr_rampup_length: float = 0.05, noise_ramp_length: float = 0.75, route: Optional[str] = None, device=None,
                 w_std: Optional[float] = None, w_avg_samples: int = 10000, draws: Optional[ClarityDraws] = None, lpips: Optional[Callable] = None):
        drawings_u8 = np.asarray(drawings_u8)
        r = gen.cfg.img_resolution
        if drawings_u8.dtype != np.uint8 or drawings_u8.ndim != 3 or drawings_u8.shape[0] < 1 or drawings_u8.shape[1:] != (r, r):
            raise ValueError(f"ClarityOptimizer: uint8 drawings [N,{r},{r}] expected, got {drawings_u8.dtype} {drawings_u8.shape}")
        if device is None:
            device = next(gen.parameters()).device if isinstance(gen, torch.nn.Module) else torch.device("cpu")
        self.gen, self.encode, self.device = gen, encode, torch.device(device)
        self.route = route if route is not None else ("hip" if self.device.type == "cuda" else "torch")
        if self.route not in ("hip", "torch"):
            raise ValueError(f"route {self.route!r}: 'hip' or 'torch'")
        if self.route == "hip" and self.device.type != "cuda":
            from ._lib import NeubeHipError
            raise NeubeHipError("route='hip' needs a GPU (there is no CPU fallback for the clarity kernels)")
        self.losses_string = losses
        self.lpips = lpips
        self.losses = ForgerLosses.create_from_string(losses, lpips)       # without a network 'lpips' raises here
        names = [l.full_name() for l in self.losses.losses]
        # the three fused items, with or without lpips(fake_orig) beside them: the perceptual term is added per brush to the fused total
        with_lpips = lpips is not None and _LPIPS_ITEM in names
        self.fused = sorted(n for n in names if not (with_lpips and n == _LPIPS_ITEM)) == sorted(_FUSED_ITEMS) and \
            not any(l.partial_loss_with_triband_input for l in self.losses.losses)
        self.fused_weights = tuple(float(self.losses.weights[names.index(n)]) for n in _FUSED_ITEMS) if self.fused else None
        self.lpips_weight = float(self.losses.weights[names.index(_LPIPS_ITEM)]) if (self.fused and with_lpips) else None
        self.item_names = (list(_FUSED_ITEMS) + ([_LPIPS_ITEM] if self.lpips_weight is not None else [])) if self.fused else names
        self.drawings = torch.from_numpy(drawings_u8).to(self.device)
        self.layout = ArenaLayout.from_config(gen.cfg)
        self.reg_weight = float(regularize_noise_weight)
        self.schedule = dict(initial_learning_rate=initial_learning_rate, initial_noise_factor=initial_noise_factor,
                             lr_rampdown_length=lr_rampdown_length, lr_rampup_length=lr_rampup_length, noise_ramp_length=noise_ramp_length)
        self.w_std, self.w_avg_samples, self.draws = w_std, w_avg_samples, draws
        self.history: Dict = {}

    # -- pieces of a step (the tests drive them one by one) --
    def noise_buffers(self, arena: torch.Tensor, b: int) -> Dict[str, torch.Tensor]:
        """{name: [K*B,1,r,r]}: brush k's planes for its B samples."""
        k, out = arena.shape[0], {}
        for i, name in enumerate(self.layout.names):
            r = self.layout.res[i]
            out[name] = self.layout.plane(arena, i).view(k, 1, 1, r, r).expand(k, b, 1, r, r).reshape(k * b, 1, r, r)
        return out

    def _ws(self, w_rows: torch.Tensor, b: int) -> torch.Tensor:
        k = w_rows.shape[0]
        return w_rows.unsqueeze(1).expand(k, b, *w_rows.shape[1:]).reshape(k * b, *w_rows.shape[1:])

    def loss_and_grad(self, arena: torch.Tensor, w_start: torch.Tensor, w_noise: torch.Tensor, geom: torch.Tensor, hip_ops: Optional[HipArenaOps] = None):
        """One evaluation at ``arena`` [K,P]: returns (grad [K,P], items [K,len(item_names)], reg [K]) of
        sum_k loss_k + regularize_noise_weight * reg_k.  ``w_start`` [K,num_ws,w_dim], ``w_noise`` likewise (already scaled),
        ``geom`` [B,1,R,R] in 0..1."""
        lo, k, b = self.layout, arena.shape[0], geom.shape[0]
        with torch.no_grad():
            feats = [f.repeat(k, 1, 1, 1) for f in self.encode(geom)]
            target, _ = self.gen.synthesis(self._ws(w_start, b), feats, noise_mode="const", noise_buffers=self.noise_buffers(arena, b),
                                           return_debug_data=True)
        a = arena.detach().clone().requires_grad_(True)
        img, raw = self.gen.synthesis(self._ws(lo.w(a) + w_noise, b), feats, noise_mode="const", noise_buffers=self.noise_buffers(a, b),
                                      return_debug_data=True)
        if self.fused and self.route == "hip":
            total, items = fused_clarity_loss(raw["uvs"], img, target, geom, k, self.fused_weights)
        elif self.fused:
            out = loss_torch(raw["uvs"], img, target, geom, k, self.fused_weights)
            total, items = out[:, 3], out[:, :3].detach()
        if self.fused and self.lpips_weight is not None:                   # the target changes every step: nothing to bind
            perc = self.lpips(target, img).reshape(k, b).mean(dim=1)
            total, items = total + self.lpips_weight * perc, torch.cat([items, perc.detach().unsqueeze(1)], dim=1)
        if not self.fused:
            total, items = [], []
            for i in range(k):                                             # brushes are independent: ForgerLosses.compute on each one's samples
                sl = slice(i * b, (i + 1) * b)
                d = {key: val[sl] for key, val in raw.items() if torch.is_tensor(val) and val.shape[0] == k * b}
                d["fake_img"], d["fake_orig"] = img[sl], target[sl]
                t_i, vals = self.losses.compute(d, geom)
                total.append(t_i)
                items.append(torch.stack([vals[n].detach() for n in self.item_names]))
            total, items = torch.stack(total), torch.stack(items)
        if self.route == "hip":
            total.sum().backward()
            grad = a.grad
            reg = (hip_ops or HipArenaOps(lo, k, self.device)).noise_reg(arena, grad, self.reg_weight)
        else:
            reg = noise_reg_torch(a, lo)
            (total.sum() + self.reg_weight * reg.sum()).backward()
            grad, reg = a.grad, reg.detach()
        return grad, items.detach(), reg

    def start_w(self, library, style_ids) -> torch.Tensor:
        """[n,num_ws,w_dim]: a seed or z goes through ``mapping``; a stored W is used as it is (broadcast over num_ws if it has one)."""
        from .painting import GanBrushOptions
        cfg, out = self.gen.cfg, []
        for sid in style_ids:
            opts = GanBrushOptions()
            library.set_style(sid, opts)
            if opts.style_z is not None:
                with torch.no_grad():
                    w = self.gen.mapping(torch.as_tensor(opts.style_z).to(self.device), None)
            else:
                w = torch.as_tensor(opts.style_ws)
            w = w.detach().to(self.device, torch.float32).reshape(1, -1, cfg.w_dim)
            out.append(w.expand(1, cfg.num_ws, cfg.w_dim) if w.shape[1] == 1 else w)
        return torch.cat(out).contiguous()

    def optimize(self, library, style_ids: Optional[Sequence] = None, num_steps: int = 1000, batch_size: int = 20, brushes_per_pass: int = 4,
                 seed: Optional[int] = None, on_step: Optional[Callable] = None) -> Dict:
        """{id: {"w": [1,num_ws,w_dim], "noise": {name: [r,r]}}} (CPU tensors; what ``WBrushLibrary._split`` reads).  ``on_step(ids, step,
        lr, items [K,n_items], reg [K])`` sees every step's values (device tensors).  ``history[id]`` keeps the first and the last."""
        ids = list(library.get_style_ids() if style_ids is None else style_ids)
        if num_steps < 1 or batch_size < 1 or brushes_per_pass < 1:
            raise ValueError("optimize: num_steps, batch_size and brushes_per_pass must be positive")
        gen, was_training, frozen = self.gen, None, []
        if isinstance(gen, torch.nn.Module):                               # no weight gradients, no w_avg update
            was_training = gen.training
            gen.eval()
            frozen = [p for p in gen.parameters() if p.requires_grad]
            for p in frozen:
                p.requires_grad_(False)
        try:
            if self.w_std is None:
                self.w_std = w_stats(gen.mapping, gen.cfg.z_dim, self.w_avg_samples, self.device)[1]
            if seed is None:
                seed = int(torch.randint(0, 2 ** 31 - 1, (1,)))
            draws = self.draws if self.draws is not None else ClarityDraws(seed, self.drawings.shape[0])
            w_all = self.start_w(library, ids)
            result: Dict = {}
            for p0 in range(0, len(ids), brushes_per_pass):
                sel = list(range(p0, min(len(ids), p0 + brushes_per_pass)))
                result.update(self._optimize_pass([ids[i] for i in sel], sel, w_all[sel], draws, num_steps, batch_size, on_step))
            return result
        finally:
            for p in frozen:
                p.requires_grad_(True)
            if was_training:
                gen.train()

    def _optimize_pass(self, ids, brush_index, w_start, draws, num_steps, batch_size, on_step):
        lo, k, dev = self.layout, len(ids), self.device
        arena = torch.empty([k, lo.p], dtype=torch.float32, device=dev)
        arena[:, :lo.nw] = w_start.reshape(k, -1)
        arena[:, lo.nw:] = torch.stack([draws.initial_noise(bi, lo.p - lo.nw) for bi in brush_index]).to(dev)
        m, v = torch.zeros_like(arena), torch.zeros_like(arena)
        hip_ops = HipArenaOps(lo, k, dev) if self.route == "hip" else None
        first = last = None
        for step in range(num_steps):
            lr, w_noise_scale = lr_and_noise_schedule(step, num_steps, self.w_std, **self.schedule)
            idx = draws.drawings(step, batch_size).to(dev)
            geom = (self.drawings[idx].to(torch.float32) / 255.0).unsqueeze(1)
            w_noise = torch.stack([draws.w_noise(step, bi, lo.w_shape) for bi in brush_index]).to(dev) * w_noise_scale
            grad, items, reg = self.loss_and_grad(arena, w_start, w_noise, geom, hip_ops)
            if self.route == "hip":
                hip_ops.step(arena, grad, m, v, lr, step + 1)
            else:
                step_torch(arena, grad, m, v, lo, lr, step + 1)
            last = (items, reg)
            first = first if first is not None else last
            if on_step is not None:
                on_step(ids, step, lr, items, reg)
        host = arena.cpu()
        rec = lambda pair, i: {**{n: float(pair[0][i, j]) for j, n in enumerate(self.item_names)}, "noise_reg": float(pair[1][i])}
        out = {}
        for i, sid in enumerate(ids):
            self.history[sid] = {"first": rec(first, i), "last": rec(last, i)}
            out[sid] = {"w": lo.w(host)[i:i + 1].clone(), "noise": {n: lo.plane(host, j)[i].clone() for j, n in enumerate(lo.names)}}
        return out
