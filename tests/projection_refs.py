"""Float64 statement of the brush projection's loss (brushstroke_engine_amd/projection.py, csrc/nb_projection.hip) and the cases its
tests share.

The statement is written from the reference's text (scripts/project_main.py:139-168, 227-250; forger/metrics/geom_metric.py:132-140;
forger/viz/visualize.py:315-323), not from the code under test:
  * ``masks_f64``: the conservative masks from a float64 double blur, the counts and the mean background colour per exemplar;
  * ``loss_f64`` (torch float64, differentiable) and ``loss_bwd_f64`` (the closed form the backward kernel evaluates);
  * ``stand_in_perceptual``: a differentiable stand-in for the LPIPS item.
Bounds of the kernel tests: ``clarity_refs.bound``."""
import numpy as np
import torch
import torch.nn.functional as F

import brush_metrics_refs as bmr
import clarity_refs as cr
from oracle import neube_oracle as orc

BG_THRESH, FG_THRESH = 0.999, 0.1
MARGIN = 1e-5                                   # no float64 blur value of a case may lie this close to a threshold (see drawings())


def _f64(a):
    return a.detach().cpu().to(torch.float64) if torch.is_tensor(a) else torch.from_numpy(np.asarray(a, np.float64))


def stand_in_perceptual(target, synth):
    return F.avg_pool2d(target - synth, 4).square().mean(dim=(1, 2, 3))


# ------------------------------------------------------------------------------------------------
# masks
# ------------------------------------------------------------------------------------------------
def drawings(r, n, seed=0):
    """[n,1,r,r] float32 in 0..1, 0 = stroke: ``clarity_refs.line_drawings`` of width 8 (with width 2 an exemplar can have no pixel whose
    blur is below 0.1).  Asserts that no float64 blur value lies within MARGIN of a threshold: nb_eval_masks_f32 is within 4e-6 of
    float64, so masks and counts must then be equal exactly, not within a tolerance."""
    g = cr.line_drawings(r, n, seed=seed, width=8).astype(np.float32) / 255.0
    blur = bmr.blur_twice(g)
    assert np.abs(blur - FG_THRESH).min() > MARGIN and np.abs(blur - BG_THRESH).min() > MARGIN
    return g[:, None]


def masks_f64(geom, target, k):
    """(mask [N,r,r] uint8: bit 0 background, bit 1 foreground; counts [k,2] = {n_fg, n_bg}; bg_color [k,3] float64, zeros without
    background) of drawings [N,1,r,r] and patches [N,3,r,r]."""
    geom, target = _f64(geom).numpy(), _f64(target).numpy()
    n = geom.shape[0]
    b = n // k
    blur = bmr.blur_twice(geom[:, 0])
    bg, fg = blur >= BG_THRESH, blur < FG_THRESH
    mask = (bg.astype(np.uint8) | (fg.astype(np.uint8) << 1))
    counts, color = np.zeros([k, 2], np.int64), np.zeros([k, 3])
    for i in range(k):
        sl = slice(i * b, (i + 1) * b)
        counts[i] = fg[sl].sum(), bg[sl].sum()
        if counts[i, 1]:
            color[i] = [target[sl, c][bg[sl]].mean() for c in range(3)]
    return mask, counts, color


def counts_of(mask, k):
    m = np.asarray(mask).reshape(k, -1)
    return np.stack([((m >> 1) & 1).sum(axis=1), (m & 1).sum(axis=1)], axis=1).astype(np.int32)


# ------------------------------------------------------------------------------------------------
# loss
# ------------------------------------------------------------------------------------------------
def loss_f64(uvs, colors, img, target, bg_image, bg_color, mask, k, composite, weights):
    """(out [k,3] = {l1, bg, weighted sum}, synth [N,3,r,r]) in torch float64; tensors that are float64 already are used as they are,
    so they may require grad."""
    as64 = lambda x: None if x is None else (x if (torch.is_tensor(x) and x.dtype == torch.float64) else _f64(x))
    uvs, colors, img, target, bg_image, bg_color = (as64(x) for x in (uvs, colors, img, target, bg_image, bg_color))
    mask = torch.from_numpy(np.asarray(mask.cpu() if torch.is_tensor(mask) else mask).astype(np.int64))
    n = uvs.shape[0]
    b = n // k
    fg, bg = ((mask >> 1) & 1).to(torch.float64), (mask & 1).to(torch.float64)
    if composite:
        synth = []
        for i in range(n):
            back = bg_image[i] if bg_image is not None else bg_color[i // b].reshape(3, 1, 1)
            stroke = torch.stack([sum(uvs[i, j] * colors[i, c, j] for j in range(3)) for c in range(3)])
            synth.append(stroke * (1 - uvs[i, 2]) + back * uvs[i, 2])
        synth = torch.stack(synth)
    else:
        synth = img
    rows = []
    for i in range(k):
        sl = slice(i * b, (i + 1) * b)
        n_fg, n_bg = fg[sl].sum(), bg[sl].sum()
        l1 = ((target[sl] - synth[sl]).abs() * fg[sl].unsqueeze(1)).sum() / (3 * n_fg) if n_fg > 0 else synth.sum() * 0
        bgv = ((1 - uvs[sl, 2]) * bg[sl]).sum() / n_bg if n_bg > 0 else synth.sum() * 0
        rows.append(torch.stack([l1, bgv, weights[0] * l1 + weights[1] * bgv]))
    return torch.stack(rows), synth


def loss_bwd_f64(uvs, colors, img, target, bg_image, bg_color, mask, k, composite, weights, d_synth=None, gscale=None):
    """(d_uvs, d_img or None, d_colors or None) numpy float64, the closed form: with G = d_synth + gscale w_l1 [fg] sign(synth - target) /
    (3 n_fg) and a = 1 - uvs[2]: d_uvs[j] = sum_c G[c] colors[c][j] a (j = 0, 1), d_uvs[2] = sum_c G[c] (colors[c][2] a - stroke[c] +
    bg[c]) - gscale w_bg [bg] / n_bg, d_colors[c][j] = sum_pixels G[c] uvs[j] a; without the composite d_img = G and only the
    background term reaches uvs."""
    np64 = lambda x: None if x is None else _f64(x).numpy()
    uvs, colors, img, target, bg_image, bg_color, d_synth = (np64(x) for x in (uvs, colors, img, target, bg_image, bg_color, d_synth))
    mask = np.asarray(mask.cpu() if torch.is_tensor(mask) else mask)
    n, r = uvs.shape[0], uvs.shape[-1]
    b = n // k
    gs = np.ones([k]) if gscale is None else np.asarray(_f64(gscale).numpy(), np.float64)
    counts = counts_of(mask, k)
    d_uvs, d_img, d_colors = np.zeros([n, 3, r, r]), None if composite else np.zeros([n, 3, r, r]), np.zeros([n, 3, 3]) if composite else None
    for i in range(n):
        e = i // b
        fg, bg = ((mask[i] >> 1) & 1).astype(np.float64), (mask[i] & 1).astype(np.float64)
        c_l1 = gs[e] * weights[0] / (3 * counts[e, 0]) if counts[e, 0] else 0.0
        c_bg = gs[e] * weights[1] / counts[e, 1] if counts[e, 1] else 0.0
        a = 1 - uvs[i, 2]
        d_uvs[i, 2] = -c_bg * bg
        for c in range(3):
            if composite:
                back = bg_image[i, c] if bg_image is not None else bg_color[e, c]
                stroke = sum(uvs[i, j] * colors[i, c, j] for j in range(3))
                synth = stroke * a + back * uvs[i, 2]
            else:
                synth = img[i, c]
            G = c_l1 * fg * np.sign(synth - target[i, c]) + (d_synth[i, c] if d_synth is not None else 0.0)
            if composite:
                for j in range(2):
                    d_uvs[i, j] += G * colors[i, c, j] * a
                d_uvs[i, 2] += G * (colors[i, c, 2] * a - stroke + back)
                for j in range(3):
                    d_colors[i, c, j] = (G * uvs[i, j] * a).sum()
            else:
                d_img[i, c] = G
    return d_uvs, d_img, d_colors


# ------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------
LOSS_CASES = [(r, b, k) for r in (8, 20, 64) for b in (1, 3) for k in (1, 2)]


def loss_case(r, b, k, composite=True, bg_image=False, seed=0, no_fg_patch=False, no_fg_exemplar=False):
    """Inputs of the loss entries as float32 numpy: softmax uvs, tanh colours and images, a random mask (about 40% foreground, 30%
    background; the entries take any mask).  On the region [: r//2, : r//3] synth equals target EXACTLY in float32 and in float64
    (sign 0): with the composite uvs = (0, 0, 1) there, so synth is the background itself and target is set to it; without, target is
    set to img.  ``no_fg_patch``: patch 0 has no foreground pixel; ``no_fg_exemplar``: the last exemplar has none."""
    rs = np.random.RandomState(7000 * r + 70 * b + 7 * k + seed + (1 if composite else 0) + (2 if bg_image else 0))
    n = k * b
    uvs = torch.softmax(torch.from_numpy(rs.randn(n, 3, r, r).astype(np.float32) * 2), dim=1).numpy()
    colors = np.tanh(rs.randn(n, 3, 3)).astype(np.float32)
    img = np.tanh(rs.randn(n, 3, r, r)).astype(np.float32)
    target = np.tanh(rs.randn(n, 3, r, r)).astype(np.float32)
    bgi = np.tanh(rs.randn(n, 3, r, r)).astype(np.float32) if (bg_image and composite) else None
    bg_color = np.tanh(rs.randn(k, 3)).astype(np.float32)
    u = rs.rand(n, r, r)
    mask = np.where(u < 0.4, 2, np.where(u < 0.7, 1, 0)).astype(np.uint8)
    if no_fg_patch:
        mask[0][mask[0] == 2] = 0
    if no_fg_exemplar:
        m = mask[(k - 1) * b:]
        m[m == 2] = 0
    h, w = r // 2, r // 3
    if composite:
        uvs[:, 0, :h, :w], uvs[:, 1, :h, :w], uvs[:, 2, :h, :w] = 0.0, 0.0, 1.0
        target[:, :, :h, :w] = bgi[:, :, :h, :w] if bgi is not None else np.repeat(bg_color, b, axis=0)[:, :, None, None]
    else:
        target[:, :, :h, :w] = img[:, :, :h, :w]
    mask[:, 0, 0] = 2                                                      # (a foreground pixel inside the sign-0 region)
    if no_fg_patch:
        mask[0, 0, 0] = 0
    if no_fg_exemplar:
        mask[(k - 1) * b:, 0, 0] = 0
    return dict(uvs=uvs, colors=colors, img=img, target=target, bg_image=bgi, bg_color=bg_color, mask=mask, counts=counts_of(mask, k),
                k=k, b=b, r=r, composite=composite, weights=(0.7, 1.3))


# ------------------------------------------------------------------------------------------------
# a differentiable generator for CPU runs, exemplars
# ------------------------------------------------------------------------------------------------
class OracleGen(cr.OracleGen):
    """``clarity_refs.OracleGen`` with the positions argument ``projection.BrushProjector`` passes."""

    def synthesis(self, ws, geom_feature, norm_noise_positions=None, noise_mode="const", noise_buffers=None, return_debug_data=False):
        assert noise_mode == "const"
        nb = noise_buffers or None
        if norm_noise_positions is None or nb is None or all(v.ndim == 2 for v in nb.values()):
            return self.o.synthesis(ws, geom_feature, return_debug_data=return_debug_data, noise_buffers=nb, norm_noise_positions=norm_noise_positions)
        outs = []                                                          # the oracle shifts one plane per layer: sample by sample
        for i in range(ws.shape[0]):
            outs.append(self.o.synthesis(ws[i:i + 1], [f[i:i + 1] for f in geom_feature], return_debug_data=True,
                                         noise_buffers={k: (v if v.ndim == 2 else v[i, 0]) for k, v in nb.items()},
                                         norm_noise_positions=norm_noise_positions[i:i + 1]))
        img = torch.cat([o[0] for o in outs])
        raw = {k: torch.cat([o[1][k] for o in outs]) for k in ("uvs", "colors")}
        return (img, raw) if return_debug_data else img


def exemplar(r, b, seed, with_bg=False, with_positions=False):
    """(target [b,3,r,r] in 0..1, geom [b,1,r,r], positions or None, target_bg or None): a flat paper colour with a darker, textured
    stroke where the drawing is."""
    rs = np.random.RandomState(seed)
    geom = drawings(r, b, seed=seed)
    paper, ink = rs.uniform(0.7, 0.95, [1, 3, 1, 1]), rs.uniform(0.05, 0.4, [1, 3, 1, 1])
    tex = 0.05 * rs.randn(b, 3, r, r)
    target = np.clip(geom * paper + (1 - geom) * (ink + tex), 0, 1).astype(np.float32)
    pos = torch.from_numpy(rs.randint(0, 4 * r, [b, 2]).astype(np.float32)) if with_positions else None
    tbg = torch.from_numpy(np.clip(paper + 0.02 * rs.randn(b, 3, r, r), 0, 1).astype(np.float32)) if with_bg else None
    return torch.from_numpy(target), torch.from_numpy(geom), pos, tbg


def run_statement_loop(gen64, encode, ex, w_start, draws, num_steps, w_std, w_plus, composite, weights, reg_weight=10.0, perceptual=None,
                       optimize_noise=True, lr0=0.1):
    """The loop of project_main.py:122-218 for ONE exemplar in float64, driven by ``draws``: per step (lr, [l1, bg, perceptual], reg, the
    smallest sqrt(v_hat) of Adam's denominators after the step), the final arena row and the row at the step whose criterion (the
    perceptual value, else the weighted sum) was lowest.  ``ex`` an exemplar 4-tuple, ``gen64`` an OracleGen of dtype float64."""
    from brushstroke_engine_amd import clarity
    cfg = gen64.cfg
    full = clarity.ArenaLayout.from_config(cfg)
    rows = cfg.num_ws if w_plus else 1
    lo = clarity.ArenaLayout(rows * cfg.w_dim, full.res if optimize_noise else [], full.names if optimize_noise else [], (rows, cfg.w_dim))
    target, geom = _f64(ex[0]) * 2 - 1, _f64(ex[1])
    b, r = geom.shape[0], geom.shape[-1]
    norm_pos = None if ex[2] is None else (_f64(ex[2]) % r) / (r - 1)
    bg_image = None if ex[3] is None else _f64(ex[3]) * 2 - 1
    mask, counts, bg_color = masks_f64(geom, target, 1)
    feats = encode(geom)
    arena = np.zeros([1, lo.p])
    arena[0, :lo.nw] = _f64(w_start).numpy().reshape(-1)
    if lo.p > lo.nw:
        arena[0, lo.nw:] = draws.initial_noise(0, lo.p - lo.nw).numpy()
    m, v, steps, best, best_row = np.zeros_like(arena), np.zeros_like(arena), [], np.inf, None
    for step in range(num_steps):
        lr, scale = cr.schedule_f64(step, num_steps, w_std, initial_learning_rate=lr0)
        a = torch.from_numpy(arena.copy()).requires_grad_(True)
        nb = {n: lo.plane(a, i).reshape(1, 1, lo.res[i], lo.res[i]).expand(b, 1, lo.res[i], lo.res[i]) for i, n in enumerate(lo.names)}
        w = lo.w(a) + _f64(draws.w_noise(step, 0, lo.w_shape)).unsqueeze(0) * scale
        ws = (w if w_plus else w.expand(1, cfg.num_ws, cfg.w_dim)).expand(b, -1, -1)
        img, raw = gen64.synthesis(ws, feats, norm_noise_positions=norm_pos, noise_buffers=nb, return_debug_data=True)
        out, synth = loss_f64(raw["uvs"], raw["colors"], img, target, bg_image, torch.from_numpy(bg_color), mask, 1, composite, weights)
        total, perc = out[0, 2], None
        if perceptual is not None:
            perc = perceptual(target, synth).mean()
            total = total + perc
        crit = float((perc if perc is not None else out[0, 2]).detach())
        if crit < best:
            best, best_row = crit, arena[0].copy()
        reg = cr.noise_reg_f64(a, lo) if lo.res else torch.zeros([1], dtype=torch.float64)
        (total + reg_weight * reg[0]).backward()
        arena, m, v = cr.step_f64(arena, a.grad.numpy(), m, v, lo, lr, step + 1)
        steps.append((lr, np.array([float(out[0, 0]), float(out[0, 1]), float(perc) if perc is not None else 0.0]), float(reg[0].detach()),
                      float(np.sqrt(v / (1 - 0.999 ** (step + 1))).min())))
    return steps, arena[0], best_row, bg_color[0]
