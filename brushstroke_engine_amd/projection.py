"""Brush projection: make a brush from a picture -- the reference's ``scripts/project_main.py`` -- for K exemplars per pass.

Given patches of an exemplar image of a medium and the drawing that goes with them, W (or W+) and the generator's noise planes are
optimised so that the generator reproduces the exemplar; the result is what ``formats.WBrushLibrary`` reads.

The state of K brushes is ``clarity.ClarityOptimizer``'s arena ``[K, P]`` (:class:`clarity.ArenaLayout`): the regulariser, Adam and the
per-plane renormalisation of ``project()`` (``project_main.py:115, 172-181, 209-218``) are the clarity entries.  The loss around the
generator -- conservative masks, mean background colour, composite, L1 over the foreground, background item -- runs, with
``route="hip"``, on the three entries of ``csrc/nb_projection.hip`` and, with ``route="torch"``, as the reference's operations in
float32 torch (what CPU tests run and what the GPU tests and ``tools/bench_projection.py`` compare against).

The reference's perceptual item is the LPIPS network: ``perceptual`` takes a :class:`perceptual.LPIPS` (no weights are shipped) or
any callable.
"""
from __future__ import annotations

from typing import Callable, Dict, Optional, Sequence

import numpy as np
import torch
import torch.nn.functional as F

from .clarity import ArenaLayout, ClarityDraws, HipArenaOps, _dense_samples, _stream, lr_and_noise_schedule, noise_reg_torch, step_torch, w_stats
from .tile_ops import gaussian_blur_torch

BG_THRESH, FG_THRESH = 0.999, 0.1          # get_conservative_fg_bg (forger/metrics/geom_metric.py:136-137)
CHECK_EVERY = 100                          # steps between two looks at the criterion (project_main.py:187)


# ------------------------------------------------------------------------------------------------
# route "torch": the reference's operations, float32 (or whatever dtype the tensors have)
# ------------------------------------------------------------------------------------------------
def conservative_masks_torch(geom: torch.Tensor):
    """(fg, bg) bool [N,1,R,R] of drawings [N,1,R,R] (0 = stroke): ``get_conservative_fg_bg`` (geom_metric.py:132-140)."""
    blur = gaussian_blur_torch(gaussian_blur_torch(geom))
    return blur < FG_THRESH, blur >= BG_THRESH


def masked_color_torch(target: torch.Tensor, bg: torch.Tensor, k: int) -> torch.Tensor:
    """[K,3]: ``compute_masked_color`` (project_main.py:248-250) of every exemplar's B patches; zeros where it has no background."""
    b = target.shape[0] // k
    rows = []
    for i in range(k):
        t, m = target[i * b:(i + 1) * b], bg[i * b:(i + 1) * b]
        rows.append(torch.stack([t[:, c:c + 1][m].mean() for c in range(3)]) if bool(m.any()) else torch.zeros([3], dtype=target.dtype, device=target.device))
    return torch.stack(rows)


def composite_torch(uvs, colors, bg):
    """``composite_with_bg_color`` / ``composite_with_bg_image`` (project_main.py:227-245); ``bg`` broadcasts against [N,3,R,R]."""
    alpha = 1 - uvs[:, 2].unsqueeze(1)
    stroke = torch.sum(uvs.unsqueeze(1) * colors.unsqueeze(-1).unsqueeze(-1), dim=2)          # compose_stroke, visualize.py:315-323
    return stroke * alpha + bg * (1 - alpha)


def loss_torch(uvs, colors, img, target, bg_image, bg_color, fg, bg, k: int, composite: bool, weights):
    """(out [K,3] = {l1, bg, w_l1 l1 + w_bg bg}, synth [N,3,R,R]) per exemplar (project_main.py:139-168) on samples n = exemplar * B +
    patch.  ``fg`` / ``bg``: bool [N,1,R,R]; ``bg_image`` [N,3,R,R] or None, then ``bg_color`` [K,3].  An item without pixels is 0."""
    n = uvs.shape[0]
    b = n // k
    if composite:
        back = bg_image if bg_image is not None else bg_color.repeat_interleave(b, dim=0).reshape(n, 3, 1, 1)
        synth = composite_torch(uvs, colors, back)
    else:
        synth = img
    fg3 = fg.expand(-1, 3, -1, -1)
    rows = []
    for i in range(k):
        sl = slice(i * b, (i + 1) * b)
        zero = synth[sl].sum() * 0
        l1 = F.l1_loss(target[sl][fg3[sl]].detach(), synth[sl][fg3[sl]]) if bool(fg[sl].any()) else zero
        bgv = (1 - uvs[sl, 2:][bg[sl]]).mean() if bool(bg[sl].any()) else zero
        rows.append(torch.stack([l1, bgv, weights[0] * l1 + weights[1] * bgv]))
    return torch.stack(rows), synth


# ------------------------------------------------------------------------------------------------
# route "hip": csrc/nb_projection.hip
# ------------------------------------------------------------------------------------------------
def _ptr(t):
    return None if t is None else t.data_ptr()


def projection_masks_hip(geom: torch.Tensor, target: torch.Tensor, k: int):
    """(mask [N,R,R] uint8, counts [K,2] int32 = {n_fg, n_bg}, bg_color [K,3]) of drawings [N,1,R,R] and patches [N,3,R,R] on the
    device: ``nb_eval_masks_f32`` for the double blur, ``nb_projection_masks_f32`` for the rest."""
    from . import _lib
    n, r = geom.shape[0], geom.shape[-1]
    assert n % k == 0 and target.shape == (n, 3, r, r) and geom.dtype == torch.float32 and target.dtype == torch.float32
    dev, b = geom.device, n // k
    g = geom.reshape(n, r, r).contiguous()
    target = _dense_samples(target)
    blur, mask = torch.empty_like(g), torch.empty([n, r, r], dtype=torch.uint8, device=dev)
    unused = torch.empty([2, n], dtype=torch.int32, device=dev)
    counts, bg_color = torch.empty([k, 2], dtype=torch.int32, device=dev), torch.empty([k, 3], dtype=torch.float32, device=dev)
    partials = torch.empty([n * _lib.NB_PROJECTION_PARTS * 8], dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().nb_eval_masks_f32(g.data_ptr(), n, r, blur.data_ptr(), mask.data_ptr(), unused[0].data_ptr(), unused[1].data_ptr(),
                                                _stream()), "eval_masks")
        _lib.check(_lib.lib().nb_projection_masks_f32(blur.data_ptr(), target.data_ptr(), target.stride(0), k, b, r, mask.data_ptr(), counts.data_ptr(),
                                                      bg_color.data_ptr(), partials.data_ptr(), _stream()), "projection_masks")
    return mask, counts, bg_color


class _FusedProjectionLoss(torch.autograd.Function):
    """The loss on ``nb_projection_loss_f32`` / ``nb_projection_loss_bwd_f32``: returns (total [K], items [K,2], synth).  Gradients flow
    through the totals AND through ``synth`` (a perceptual item's) to ``uvs`` and ``colors`` -- or, without the composite, through the
    totals to ``uvs`` and ``img`` (``synth`` is then an empty tensor: the perceptual item differentiates ``img`` itself)."""

    @staticmethod
    def forward(ctx, uvs, colors, img, target, bg_image, bg_color, mask, counts, k, composite, weights):
        from . import _lib
        n, r = uvs.shape[0], uvs.shape[-1]
        b, dev = n // k, uvs.device
        assert n == k * b and uvs.shape == (n, 3, r, r) and uvs.dtype == torch.float32 and target.shape == uvs.shape
        uvs, target = _dense_samples(uvs.detach()), _dense_samples(target.detach())
        if composite:
            colors = colors.detach().to(torch.float32).contiguous()
            bg_image = None if bg_image is None else _dense_samples(bg_image.detach())
            img = None
            synth = torch.empty([n, 3, r, r], dtype=torch.float32, device=dev)
        else:
            img, colors, bg_image = _dense_samples(img.detach()), None, None
            synth = torch.empty([0], dtype=torch.float32, device=dev)
        out = torch.empty([k, 3], dtype=torch.float32, device=dev)
        partials = torch.empty([n * _lib.NB_PROJECTION_PARTS * 16], dtype=torch.float32, device=dev)
        stride = lambda t: 0 if t is None else t.stride(0)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().nb_projection_loss_f32(uvs.data_ptr(), uvs.stride(0), _ptr(colors), _ptr(img), stride(img), target.data_ptr(),
                                                         target.stride(0), _ptr(bg_image), stride(bg_image), _ptr(bg_color), mask.data_ptr(),
                                                         counts.data_ptr(), k, b, r, int(composite), weights[0], weights[1],
                                                         synth.data_ptr() if composite else None, out.data_ptr(), partials.data_ptr(), _stream()),
                       "projection_loss")
        ctx.save_for_backward(uvs, colors, img, target, bg_image, bg_color, mask, counts, partials)
        ctx.k, ctx.composite, ctx.weights = k, composite, weights
        ctx.set_materialize_grads(False)
        total, items = out[:, 2].clone(), out[:, :2].clone()
        ctx.mark_non_differentiable(items)
        return total, items, synth

    @staticmethod
    def backward(ctx, g_total, _g_items, g_synth):
        from . import _lib
        uvs, colors, img, target, bg_image, bg_color, mask, counts, partials = ctx.saved_tensors
        k, composite, w = ctx.k, ctx.composite, ctx.weights
        n, r = uvs.shape[0], uvs.shape[-1]
        dev = uvs.device
        gscale = (torch.zeros([k], dtype=torch.float32, device=dev) if g_total is None else g_total.to(torch.float32)).contiguous()
        d_synth = g_synth.to(torch.float32).contiguous() if (composite and g_synth is not None) else None
        d_uvs = torch.empty([n, 3, r, r], dtype=torch.float32, device=dev)
        d_img = None if composite else torch.empty([n, 3, r, r], dtype=torch.float32, device=dev)
        d_colors = torch.empty([n, 3, 3], dtype=torch.float32, device=dev) if composite else None
        stride = lambda t: 0 if t is None else t.stride(0)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().nb_projection_loss_bwd_f32(uvs.data_ptr(), uvs.stride(0), _ptr(colors), _ptr(img), stride(img), target.data_ptr(),
                                                             target.stride(0), _ptr(bg_image), stride(bg_image), _ptr(bg_color), mask.data_ptr(),
                                                             counts.data_ptr(), _ptr(d_synth), gscale.data_ptr(), k, n // k, r, int(composite),
                                                             w[0], w[1], d_uvs.data_ptr(), _ptr(d_img), _ptr(d_colors), partials.data_ptr(),
                                                             _stream()), "projection_loss_bwd")
        return d_uvs, d_colors, d_img, None, None, None, None, None, None, None, None


def fused_projection_loss(uvs, colors, img, target, bg_image, bg_color, mask, counts, k: int, composite: bool, weights):
    """(total [K], items [K,2] = {l1, bg}, synth [N,3,R,R]) on the HIP kernels; ``mask`` / ``counts`` / ``bg_color`` from
    :func:`projection_masks_hip`.  ``synth`` is ``img`` itself without the composite."""
    total, items, synth = _FusedProjectionLoss.apply(uvs, colors if composite else None, None if composite else img, target,
                                                     bg_image if composite else None, bg_color, mask, counts, int(k), bool(composite),
                                                     tuple(float(x) for x in weights))
    return total, items, (synth if composite else img)


# ------------------------------------------------------------------------------------------------
# the loop
# ------------------------------------------------------------------------------------------------
class BrushProjector:
    """``project()`` plus ``run_projection()`` (project_main.py:38-224, 395-492) for K exemplars per pass.

    ``gen``: a differentiable generator with ``cfg``, ``mapping(z, None)`` and ``synthesis(ws, geom_feature, norm_noise_positions=...,
    noise_mode="const", noise_buffers=..., return_debug_data=True)`` -- ``training.TrainableGenerator`` on the GPU.  ``encode``:
    [N,1,R,R] float drawings (0 = stroke) -> the list of geometry features.

    An exemplar is ``(target [B,3,R,R] in 0..1, geom [B,1,R,R] in 0..1 with 0 = stroke, positions [B,2] or None, target_bg [B,3,R,R] in
    0..1 or None)``; the exemplars of one call have the same B.  A pass encodes its K*B drawings once (the patches are fixed for the
    run); a step is one generator batch of K*B samples, the loss, the noise regulariser and the Adam step with renormalisation.

    ``perceptual``: any differentiable callable ``(target, synth) -> [N]`` on images in -1..1 (the plug for the reference's
    ``lpips_batched_vgg``: a :class:`perceptual.LPIPS` loaded from a user's weight files; none ship), averaged over an exemplar's
    patches and weighted ``perceptual_weight``.  One that has ``bind(target)`` is bound to the pass's fixed target in ``prepare``.

    Departures from the reference.  (1) The best state (project_main.py:159-162) is kept by the perceptual value when there is a
    perceptual item, as there; WITHOUT one the criterion is ``l1_fg_weight * l1 + bg_weight * bg``.  (2) The early stop (:187-207)
    is per brush: a brush whose criterion improved by less than ``min_improvement`` between two checks is finished (its best row is
    frozen, its ``step`` recorded); the pass ends when all its brushes are.  (3) ``resume_from`` ({id: {"w": ...}}) supplies W; the
    noise planes restart from fresh draws, as in the reference, whose ``project()`` overwrites the planes it resumed (:105-120).
    ``history[id]["last"]`` holds the items of the step a brush finished at (its row of the arena is still stepped until the pass
    ends; nothing of it is used).  (4) An exemplar without foreground (with ``l1_fg_weight > 0``) or without background (with ``bg_weight > 0``, or with the
    composite over the mean colour) is a ``ValueError``; the reference computes NaN there."""

    def __init__(self, gen, encode: Callable, route: Optional[str] = None, perceptual: Optional[Callable] = None, perceptual_weight: float = 1.0,
                 num_steps: int = 1000, w_plus: bool = False, optimize_noise: bool = True, with_positions: bool = False, with_composite: bool = False,
                 l1_fg_weight: float = 0.0, bg_weight: float = 0.0, regularize_noise_weight: float = 10, initial_learning_rate: float = 0.1,
                 initial_noise_factor: float = 0.05, lr_rampdown_length: float = 0.25, lr_rampup_length: float = 0.05, noise_ramp_length: float = 0.75,
                 w_avg=None, w_std: Optional[float] = None, w_avg_samples: int = 10000, resume_from: Optional[Dict] = None,
                 min_improvement: float = 0.0001, device=None, draws: Optional[ClarityDraws] = None):
        if device is None:
            device = next(gen.parameters()).device if isinstance(gen, torch.nn.Module) else torch.device("cpu")
        self.gen, self.encode, self.device = gen, encode, torch.device(device)
        self.route = route if route is not None else ("hip" if self.device.type == "cuda" else "torch")
        if self.route not in ("hip", "torch"):
            raise ValueError(f"route {self.route!r}: 'hip' or 'torch'")
        if self.route == "hip" and self.device.type != "cuda":
            from ._lib import NeubeHipError
            raise NeubeHipError("route='hip' needs a GPU (there is no CPU fallback for the projection kernels)")
        if l1_fg_weight < 0 or bg_weight < 0 or num_steps < 1:
            raise ValueError("BrushProjector: weights must not be negative and num_steps must be positive")
        if perceptual is None and not (l1_fg_weight > 0 or bg_weight > 0):
            raise ValueError("BrushProjector: without a perceptual item at least one of l1_fg_weight, bg_weight must be positive")
        self.perceptual, self.perceptual_weight = perceptual, float(perceptual_weight)
        self.num_steps, self.w_plus, self.optimize_noise = int(num_steps), bool(w_plus), bool(optimize_noise)
        self.with_positions, self.with_composite = bool(with_positions), bool(with_composite)
        self.weights = (float(l1_fg_weight), float(bg_weight))
        self.reg_weight = float(regularize_noise_weight)
        self.schedule = dict(initial_learning_rate=initial_learning_rate, initial_noise_factor=initial_noise_factor,
                             lr_rampdown_length=lr_rampdown_length, lr_rampup_length=lr_rampup_length, noise_ramp_length=noise_ramp_length)
        self.w_avg, self.w_std, self.w_avg_samples = w_avg, w_std, int(w_avg_samples)
        self.resume_from, self.min_improvement, self.draws = resume_from or {}, float(min_improvement), draws
        cfg = gen.cfg
        rows = cfg.num_ws if self.w_plus else 1
        full = ArenaLayout.from_config(cfg)
        self.layout = ArenaLayout(rows * cfg.w_dim, full.res if self.optimize_noise else [], full.names if self.optimize_noise else [], (rows, cfg.w_dim))
        self.item_names = ["l1", "bg"] + (["perceptual"] if perceptual is not None else [])
        self.history: Dict = {}
        self.last_rows: Dict = {}                                          # {id: the arena row [P] after the last step} (CPU)

    # -- pieces of a step (the tests drive them one by one) --
    def noise_buffers(self, arena: torch.Tensor, b: int) -> Dict[str, torch.Tensor]:
        """{name: [K*B,1,r,r]}: brush k's planes for its B samples (empty without ``optimize_noise``: the generator's own planes)."""
        k, out = arena.shape[0], {}
        for i, name in enumerate(self.layout.names):
            r = self.layout.res[i]
            out[name] = self.layout.plane(arena, i).view(k, 1, 1, r, r).expand(k, b, 1, r, r).reshape(k * b, 1, r, r)
        return out

    def _ws(self, w_rows: torch.Tensor, b: int) -> torch.Tensor:
        """[K, rows, w_dim] -> [K*B, num_ws, w_dim] (project_main.py:135)."""
        k, cfg = w_rows.shape[0], self.gen.cfg
        w = w_rows if self.w_plus else w_rows.expand(k, cfg.num_ws, cfg.w_dim)
        return w.unsqueeze(1).expand(k, b, cfg.num_ws, cfg.w_dim).reshape(k * b, cfg.num_ws, cfg.w_dim)

    def prepare(self, exemplars: Sequence) -> Dict:
        """The fixed part of a pass: tensors on the device in the reference's ranges (run_projection, :421-431), the geometry features,
        masks, counts and mean background colours.  ``exemplars``: a list of the 4-tuples."""
        dev, r, k = self.device, self.gen.cfg.img_resolution, len(exemplars)
        t32 = lambda x: torch.as_tensor(np.asarray(x) if not torch.is_tensor(x) else x).to(dev, torch.float32)
        b = int(exemplars[0][0].shape[0])
        for tg, ge, pos, tb in exemplars:
            if tuple(tg.shape) != (b, 3, r, r) or tuple(ge.shape) != (b, 1, r, r) or (tb is not None and tuple(tb.shape) != (b, 3, r, r)) or \
                    (pos is not None and tuple(pos.shape) != (b, 2)):
                raise ValueError(f"BrushProjector: an exemplar is (target [{b},3,{r},{r}], geom [{b},1,{r},{r}], positions [{b},2] or None, target_bg "
                                 f"like target or None); got {tuple(tg.shape)}, {tuple(ge.shape)}")
        with_bg = [e[3] is not None for e in exemplars]
        if any(with_bg) and not all(with_bg):
            raise ValueError("BrushProjector: the exemplars of a pass have a target_bg all or none")
        target = torch.cat([t32(e[0]) for e in exemplars]) * 2 - 1
        geom = torch.cat([t32(e[1]) for e in exemplars])
        target_bg = torch.cat([t32(e[3]) for e in exemplars]) * 2 - 1 if all(with_bg) else None
        norm_pos = None
        if self.with_positions:
            if any(e[2] is None for e in exemplars):
                raise ValueError("BrushProjector: with_positions needs the positions of every exemplar")
            pos = torch.cat([t32(e[2]) for e in exemplars])
            norm_pos = (pos % r) / (r - 1)
        with torch.no_grad():
            feats = [f.detach() for f in self.encode(geom)]
            if self.route == "hip":
                mask, counts, bg_color = projection_masks_hip(geom, target, k)
                fix = dict(mask=mask, counts=counts)
                counts_host = counts.cpu().numpy()
            else:
                fg, bg = conservative_masks_torch(geom)
                bg_color = masked_color_torch(target, bg, k)
                fix = dict(fg=fg, bg=bg)
                counts_host = np.stack([fg.reshape(k, -1).sum(dim=1).cpu().numpy(), bg.reshape(k, -1).sum(dim=1).cpu().numpy()], axis=1)
        fix.update(k=k, b=b, target=target, geom=geom, target_bg=target_bg, norm_pos=norm_pos, feats=feats, bg_color=bg_color, counts_host=counts_host)
        # a perceptual item that can bind (perceptual.LPIPS) takes the fixed target through its trunk once per pass, here
        fix["perceptual"] = self.perceptual.bind(target) if hasattr(self.perceptual, "bind") else self.perceptual
        return fix

    def check_counts(self, ids, counts_host, has_bg_image: bool) -> None:
        for sid, (n_fg, n_bg) in zip(ids, counts_host):
            if n_fg == 0 and self.weights[0] > 0:
                raise ValueError(f"exemplar {sid!r}: no pixel of its drawings is foreground (blur < {FG_THRESH}) and l1_fg_weight > 0")
            if n_bg == 0 and (self.weights[1] > 0 or (self.with_composite and not has_bg_image)):
                raise ValueError(f"exemplar {sid!r}: no pixel of its drawings is background (blur >= {BG_THRESH}) and bg_weight > 0 or the "
                                 f"composite needs the mean background colour")

    def loss(self, raw, img, fix):
        """(total [K] to differentiate, items [K, len(item_names)] detached, criterion [K] detached) of one generator output."""
        k, b = fix["k"], fix["b"]
        if self.route == "hip":
            total, items, synth = fused_projection_loss(raw["uvs"], raw.get("colors"), img, fix["target"], fix["target_bg"], fix["bg_color"],
                                                        fix["mask"], fix["counts"], k, self.with_composite, self.weights)
        else:
            out, synth = loss_torch(raw["uvs"], raw.get("colors"), img, fix["target"], fix["target_bg"], fix["bg_color"], fix["fg"], fix["bg"], k,
                                    self.with_composite, self.weights)
            total, items = out[:, 2], out[:, :2].detach()
        crit = total.detach()
        if self.perceptual is not None:
            perc = fix.get("perceptual", self.perceptual)(fix["target"], synth).reshape(k, b).mean(dim=1)
            total = total + self.perceptual_weight * perc
            crit = perc.detach()
            items = torch.cat([items, crit.unsqueeze(1)], dim=1)
        return total, items.detach(), crit

    def loss_and_grad(self, arena: torch.Tensor, w_noise: torch.Tensor, fix: Dict, hip_ops: Optional[HipArenaOps] = None):
        """One evaluation at ``arena`` [K,P]: (grad [K,P], items, reg [K], criterion [K]) of sum_k loss_k + regularize_noise_weight *
        reg_k.  ``w_noise`` [K, rows, w_dim], already scaled."""
        lo, k, b = self.layout, arena.shape[0], fix["b"]
        a = arena.detach().clone().requires_grad_(True)
        img, raw = self.gen.synthesis(self._ws(lo.w(a) + w_noise, b), fix["feats"], norm_noise_positions=fix["norm_pos"], noise_mode="const",
                                      noise_buffers=self.noise_buffers(a, b), return_debug_data=True)
        total, items, crit = self.loss(raw, img, fix)
        if self.route == "hip":
            total.sum().backward()
            grad = a.grad
            reg = (hip_ops or HipArenaOps(lo, k, self.device)).noise_reg(arena, grad, self.reg_weight)
        else:
            reg = noise_reg_torch(a, lo)
            (total.sum() + self.reg_weight * reg.sum()).backward()
            grad, reg = a.grad, reg.detach()
        return grad, items, reg, crit

    def start_w(self, ids) -> torch.Tensor:
        """[n, rows, w_dim]: ``w_avg`` (repeated over num_ws for W+, project_main.py:84-88), or the W of ``resume_from[id]`` (:91-96)."""
        cfg, rows = self.gen.cfg, self.layout.w_shape[0]
        avg = torch.as_tensor(np.asarray(self.w_avg)).to(torch.float32).reshape(1, 1, cfg.w_dim).expand(1, rows, cfg.w_dim)
        out = []
        for sid in ids:
            entry = self.resume_from.get(sid)
            if entry is not None and "w" in entry:
                w = torch.as_tensor(entry["w"]).detach().to(torch.float32).reshape(1, -1, cfg.w_dim)
                if w.shape[1] not in (1, rows):
                    raise ValueError(f"resume_from[{sid!r}]: w of {w.shape[1]} rows, 1 or {rows} expected")
                out.append(w.expand(1, rows, cfg.w_dim))
            else:
                out.append(avg)
        return torch.cat(out).to(self.device).contiguous()

    def project(self, exemplars: Dict, brushes_per_pass: int = 4, seed: Optional[int] = None, on_step: Optional[Callable] = None) -> Dict:
        """{id: {"w": [1, num_ws or 1, w_dim], "noise": {name: [r,r]}, "bg": [3], "step": int}} (CPU tensors: the reference's result
        dictionary, which ``formats.WBrushLibrary`` reads).  ``on_step(ids, step, lr, items, reg)`` sees every step's values (device
        tensors); ``history[id]`` keeps the first and the last."""
        ids = list(exemplars)
        if not ids or brushes_per_pass < 1:
            raise ValueError("project: at least one exemplar and brushes_per_pass >= 1")
        gen, was_training, frozen = self.gen, None, []
        if isinstance(gen, torch.nn.Module):                               # no weight gradients (run_projection, :417)
            was_training = gen.training
            gen.eval()
            frozen = [p for p in gen.parameters() if p.requires_grad]
            for p in frozen:
                p.requires_grad_(False)
        try:
            if self.w_std is None or self.w_avg is None:
                self.w_avg, self.w_std = w_stats(gen.mapping, gen.cfg.z_dim, self.w_avg_samples, self.device)
            if seed is None:
                seed = int(torch.randint(0, 2 ** 31 - 1, (1,)))
            draws = self.draws if self.draws is not None else ClarityDraws(seed, 0)
            w_all = self.start_w(ids)
            result: Dict = {}
            for p0 in range(0, len(ids), brushes_per_pass):
                sel = list(range(p0, min(len(ids), p0 + brushes_per_pass)))
                result.update(self._pass([ids[i] for i in sel], sel, [exemplars[ids[i]] for i in sel], w_all[sel], draws, on_step))
            return result
        finally:
            for p in frozen:
                p.requires_grad_(True)
            if was_training:
                gen.train()

    def _pass(self, ids, brush_index, exemplars, w_start, draws, on_step):
        lo, k, dev = self.layout, len(ids), self.device
        fix = self.prepare(exemplars)
        self.check_counts(ids, fix["counts_host"], fix["target_bg"] is not None)
        arena = torch.empty([k, lo.p], dtype=torch.float32, device=dev)
        arena[:, :lo.nw] = w_start.reshape(k, -1)
        if lo.p > lo.nw:
            arena[:, lo.nw:] = torch.stack([draws.initial_noise(bi, lo.p - lo.nw) for bi in brush_index]).to(dev)
        m, v = torch.zeros_like(arena), torch.zeros_like(arena)
        hip_ops = HipArenaOps(lo, k, dev) if self.route == "hip" else None
        best_arena = arena.clone()
        best = torch.full([k], float("inf"), dtype=torch.float32, device=dev)
        finished = torch.zeros([k], dtype=torch.bool, device=dev)
        prev, done_host, steps = None, np.zeros([k], bool), np.full([k], self.num_steps - 1, np.int64)
        first = last = None
        for step in range(self.num_steps):
            lr, w_noise_scale = lr_and_noise_schedule(step, self.num_steps, self.w_std, **self.schedule)
            w_noise = torch.stack([draws.w_noise(step, bi, lo.w_shape) for bi in brush_index]).to(dev) * w_noise_scale
            grad, items, reg, crit = self.loss_and_grad(arena, w_noise, fix, hip_ops)
            better = (crit < best) & ~finished                             # project_main.py:159-162, on the device
            best = torch.where(better, crit, best)
            best_arena = torch.where(better.unsqueeze(1), arena, best_arena)
            # (a finished brush keeps the items of the step it finished at: its row is still stepped with the pass, but nothing of it is used)
            last = (items, reg) if last is None else (torch.where(finished.unsqueeze(1), last[0], items), torch.where(finished, last[1], reg))
            first = first if first is not None else last
            if on_step is not None:
                on_step(ids, step, lr, items, reg)
            if step % CHECK_EVERY == 0:                                    # :187-207, the one read-back
                now = best.cpu().numpy().astype(np.float64)
                if prev is not None:
                    stop = ~done_host & (prev - now < self.min_improvement)
                    steps[stop] = step
                    done_host |= stop
                    finished = torch.from_numpy(done_host).to(dev)
                    if done_host.all():
                        break
                prev = now
            if self.route == "hip":
                hip_ops.step(arena, grad, m, v, lr, step + 1)
            else:
                step_torch(arena, grad, m, v, lo, lr, step + 1)
        host, bg_host, last_host = best_arena.cpu(), fix["bg_color"].cpu(), arena.cpu()
        rec = lambda pair, i: {**{n: float(pair[0][i, j]) for j, n in enumerate(self.item_names)}, "noise_reg": float(pair[1][i])}
        out = {}
        for i, sid in enumerate(ids):
            self.history[sid] = {"first": rec(first, i), "last": rec(last, i)}
            self.last_rows[sid] = last_host[i].clone()
            out[sid] = {"w": lo.w(host)[i:i + 1].clone(), "noise": {n: lo.plane(host, j)[i].clone() for j, n in enumerate(lo.names)},
                        "bg": bg_host[i].clone(), "step": int(steps[i])}
        return out


# ------------------------------------------------------------------------------------------------
# patch samplers (project_main.py:253-357), on the host with a seeded numpy generator
# ------------------------------------------------------------------------------------------------
def _resize(patch: np.ndarray, width: int) -> np.ndarray:
    """[h,w,C] float32 -> [width,width,C].  The reference resizes with skimage; here it is torch's antialiased bilinear interpolation,
    so patches differ from the reference's in the resampling, not in the boxes."""
    t = torch.from_numpy(np.ascontiguousarray(patch, dtype=np.float32)).permute(2, 0, 1).unsqueeze(0)
    lo, hi = float(t.min()), float(t.max())                                # (the weights sum to 1 only up to rounding: keep the range)
    t = F.interpolate(t, size=(width, width), mode="bilinear", antialias=True, align_corners=False).clamp_(lo, hi)
    return t[0].permute(1, 2, 0).numpy()


def _fixed_patch(img, start_col, start_row, rwidth, rheight, width):
    return _resize(img[start_row:start_row + rheight, start_col:start_col + rwidth, :], width)


def _random_patch_size(shape, patch_range, rng) -> int:
    """``RandomPatchGenerator.get_random_patch_size`` (forger/util/img_proc.py:325-334): both ends included."""
    min_dim = min(shape[0], shape[1])
    lo, hi = min(min_dim, int(patch_range[0] * min_dim)), min(min_dim, int(patch_range[1] * min_dim))
    return int(rng.integers(lo, hi + 1))


def _random_box(shape, patch_range, rng):
    rwidth = _random_patch_size(shape, patch_range, rng)
    start_row, start_col = int(rng.integers(0, shape[0] - rwidth + 1)), int(rng.integers(0, shape[1] - rwidth + 1))
    return [start_col, start_row, rwidth, rwidth]


def _positions(boxes, width, patch_range, min_dim) -> torch.Tensor:
    """project_main.py:288-289, 342-343: the boxes' corners (column, row) in units of the smallest patch."""
    return torch.tensor([x[:2] for x in boxes]) * width / (patch_range[0] * min_dim)


def load_target(target_img, geom_img, width: int, crop_n: int = 10, patch_range=(0.2, 0.5), rng=None, overfit_one: bool = False, return_boxes=False):
    """``load_target`` (project_main.py:305-357): (target [N,3,W,W], geom [N,1,W,W], positions [N,2]) in 0..1 from an exemplar image
    [H,W,3+] and its geometry image [H,W,3+] (channel 1 is read), both uint8 or float in 0..1.  ``overfit_one``: one random box
    shifted up and down, plus the transposed patches (N is then not ``crop_n``)."""
    rng = rng if rng is not None else np.random.default_rng()
    to01 = lambda a: np.asarray(a).astype(np.float32) / 255.0 if np.asarray(a).dtype == np.uint8 else np.asarray(a, np.float32)
    target, geom = to01(target_img)[..., :3], to01(geom_img)
    if target.shape[:2] != geom.shape[:2]:
        raise ValueError(f"load_target: the exemplar is {target.shape[:2]}, its geometry image {geom.shape[:2]}")
    if target.shape[0] == width and target.shape[1] == width:
        raise NotImplementedError("load_target: an exemplar of exactly the patch size (as in the reference)")
    min_dim = min(target.shape[0], target.shape[1])
    if overfit_one:
        patch = _random_box(target.shape, patch_range, rng)
        half = crop_n // 2
        pheight = patch[2]
        up_space, down_space = min(patch[1], pheight // 2), min(target.shape[0] - patch[1] - pheight, pheight // 2)
        boxes = [[patch[0], patch[1] - int(up_space / half * 2 * i), patch[2], patch[3]] for i in range(half // 2, 1, -1)]
        boxes.append(patch)
        boxes += [[patch[0], patch[1] + int(down_space / half * 2 * i), patch[2], patch[3]] for i in range(1, half // 2)]
    else:
        boxes = [_random_box(target.shape, patch_range, rng) for _ in range(crop_n)]
    tp = torch.from_numpy(np.stack([_fixed_patch(target, *x, width) for x in boxes])).permute(0, 3, 1, 2)
    gp = torch.from_numpy(np.stack([_fixed_patch(geom, *x, width) for x in boxes])).permute(0, 3, 1, 2)[:, 1:2]
    positions = _positions(boxes, width, patch_range, min_dim)
    if overfit_one:                                                        # flip augmentation
        tp, gp = torch.cat([tp, tp.permute(0, 1, 3, 2)]), torch.cat([gp, gp.permute(0, 1, 3, 2)])
        positions = torch.cat([positions, positions])
    out = (tp.contiguous(), gp.contiguous(), positions)
    return out + (boxes,) if return_boxes else out


def load_target_sparse(target_img, target_bg_img, geom_img, width: int, crop_n: int = 10, patch_range=(0.2, 0.5), rng=None, return_boxes=False):
    """``load_target_sparse`` (project_main.py:253-302): boxes around stroke pixels, kept when more than 5% of the box is stroke;
    (target, target_bg or None, geom, positions).  ``geom_img`` uint8 (0 = stroke exactly, as the reference tests).  The reference's
    retry loop does not terminate as written (``or ntries > crop_n * 10``); here at most ``crop_n * 10`` centres are tried and a
    ``ValueError`` follows when they do not yield ``crop_n`` boxes."""
    rng = rng if rng is not None else np.random.default_rng()
    target = np.asarray(target_img)[..., :3].astype(np.float32) / 255.0
    geom_u8 = np.asarray(geom_img)[..., 1:2]
    if target.shape[:2] != geom_u8.shape[:2]:
        raise ValueError(f"load_target_sparse: the exemplar is {target.shape[:2]}, its geometry image {geom_u8.shape[:2]}")
    min_dim = min(target.shape[0], target.shape[1])
    zeros = np.where(geom_u8 == 0)
    yx = np.stack([zeros[0], zeros[1]], axis=1)
    yx = yx[rng.permutation(len(yx))]
    geom = geom_u8.astype(np.float32) / 255.0
    boxes, ntries = [], 0
    while len(boxes) < crop_n and ntries < min(len(yx), crop_n * 10):
        pcenter = yx[ntries]
        ntries += 1
        rwidth = _random_patch_size(target.shape, patch_range, rng)
        start_row, start_col = max(0, int(pcenter[0]) - rwidth // 2), max(0, int(pcenter[1]) - rwidth // 2)
        res_patch = geom[start_row:start_row + rwidth, start_col:start_col + rwidth, 0]
        if np.sum(res_patch < 0.1) > rwidth * rwidth * 0.05:
            boxes.append([start_col, start_row, rwidth, rwidth])
    if len(boxes) < crop_n:
        raise ValueError(f"load_target_sparse: {ntries} centres gave {len(boxes)} of {crop_n} boxes with enough stroke")
    stack = lambda img: torch.from_numpy(np.stack([_fixed_patch(img, *x, width) for x in boxes])).permute(0, 3, 1, 2).contiguous()
    bgp = None
    if target_bg_img is not None:
        target_bg = np.asarray(target_bg_img)[..., :3].astype(np.float32) / 255.0
        bgp = stack(target * geom + target_bg * (1 - geom))
    out = (stack(target), bgp, stack(geom), _positions(boxes, width, patch_range, min_dim))
    return out + (boxes,) if return_boxes else out
