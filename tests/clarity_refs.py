"""Float64 statement of the clarity optimisation (brushstroke_engine_amd/clarity.py, csrc/nb_clarity.hip) and the cases its tests share.

The statement is written sample by sample and plane by plane, from the reference's text (forger/train/losses.py:453-474, 501-530,
649-666; scripts/opt_clarity_main.py:94-100, 127-137, 159-167), not from the code under test:
  * ``loss_f64`` (torch float64, differentiable) and ``loss_bwd_f64`` (the closed form the backward kernel evaluates);
  * ``noise_reg_f64`` (torch float64, differentiable) and ``noise_reg_grad_f64`` (the closed form);
  * ``step_f64`` (Adam with bias correction, then the per-plane renormalisation);
  * ``schedule_f64``.
Bounds of the kernel tests: ``bound()``."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from brushstroke_engine_amd import clarity
from oracle import neube_oracle as orc

# A kernel sums in another order than torch does: its error may exceed the float32 torch route's, measured on the same inputs against
# float64, by this factor -- and is never asked to be below ULP_FLOOR float32 ulps of the value itself.
BOUND_FACTOR = 4.0
ULP_FLOOR = 4.0
EPS32 = float(np.finfo(np.float32).eps)

REG_TABLE = [4, 8, 8, 16, 16, 32, 32, 64, 64, 128]
REG_NW = 40                                     # a W+ part that is no multiple of a chunk or a vector


def bound(torch32, f64, value=None):
    """Elementwise bound for a kernel result: BOUND_FACTOR x the largest error of the float32 torch route, plus ULP_FLOOR ulps of |value|."""
    f64 = np.asarray(f64, np.float64)
    e = float(np.abs(np.asarray(torch32, np.float64) - f64).max()) if np.size(f64) else 0.0
    return BOUND_FACTOR * e + ULP_FLOOR * EPS32 * np.abs(f64 if value is None else np.asarray(value, np.float64))


def mean_square_tol(r):
    """|mean(n^2) - 1| of a renormalised float32 plane of side r: the scale carries a few ulps of the variance estimate (twice that in
    the mean square) and the sums of r^2 terms are pairwise, log2(r^2) levels deep."""
    return (8 + 2 * math.log2(r * r)) * EPS32


def _f64(a):
    return a.detach().to(torch.float64) if torch.is_tensor(a) else torch.from_numpy(np.asarray(a, np.float64))


# ------------------------------------------------------------------------------------------------
# loss
# ------------------------------------------------------------------------------------------------
def loss_f64(uvs, img, target, geom, k, weights):
    """([K,4] = iou_inv(uvs), iou(u), l1(fake_orig), weighted total; per-sample sums [K*B,4] = I_s, U_s, I_u, U_u), torch float64.
    Pass tensors that require grad to differentiate."""
    uvs, img, target, geom = (x if (torch.is_tensor(x) and x.dtype == torch.float64) else _f64(x) for x in (uvs, img, target, geom))
    b, rows, sums = geom.shape[0], [], []
    for i in range(k):
        inv = iou = 0.0
        for j in range(b):
            n = i * b + j
            g = geom[j, 0]
            t = 1 - g
            s, u = uvs[n, 2], uvs[n, 0]
            i_s = (s * g).sum()
            u_s = (s + g).sum() - i_s + 1e-8
            i_u = (u * t).sum()
            u_u = (u + t).sum() - i_u + 1e-8
            inv, iou = inv + i_s / u_s, iou + i_u / u_u
            sums.append(torch.stack([i_s, u_s, i_u, u_u]))
        items = [1 - inv / b, 1 - iou / b, (img[i * b:(i + 1) * b] - target[i * b:(i + 1) * b].detach()).abs().mean()]
        rows.append(torch.stack(items + [weights[0] * items[0] + weights[1] * items[1] + weights[2] * items[2]]))
    return torch.stack(rows), torch.stack(sums)


def loss_bwd_f64(img, target, geom, sums, k, weights, gscale=None):
    """(d_uvs, d_img) of sum_k gscale_k total_k, the closed form: background channel -w/B (g U - I (1 - g)) / U^2, foreground channel
    the same with t = 1 - g, channel 1 zero, image w sign(img - target) / (B 3 r^2)."""
    img, target, geom, sums = (_f64(x).numpy() for x in (img, target, geom, sums))
    b, r = geom.shape[0], geom.shape[-1]
    gs = np.ones([k]) if gscale is None else np.asarray(gscale, np.float64)
    d_uvs, d_img = np.zeros([k * b, 3, r, r]), np.zeros([k * b, 3, r, r])
    for n in range(k * b):
        g = geom[n % b, 0]
        t = 1 - g
        i_s, u_s, i_u, u_u = sums[n]
        d_uvs[n, 2] = -weights[0] * gs[n // b] / b * (g * u_s - i_s * (1 - g)) / u_s ** 2
        d_uvs[n, 0] = -weights[1] * gs[n // b] / b * (t * u_u - i_u * (1 - t)) / u_u ** 2
        d_img[n] = weights[2] * gs[n // b] * np.sign(img[n] - target[n]) / (b * 3 * r * r)
    return d_uvs, d_img


# ------------------------------------------------------------------------------------------------
# regulariser
# ------------------------------------------------------------------------------------------------
def noise_reg_f64(arena, layout):
    """[K] torch float64 (differentiable when ``arena`` is a float64 tensor that requires grad)."""
    arena = arena if (torch.is_tensor(arena) and arena.dtype == torch.float64) else _f64(arena)
    out = []
    for k in range(arena.shape[0]):
        reg = 0.0
        for r, o in zip(layout.res, layout.off):
            noise = arena[k, o:o + r * r].reshape(1, 1, r, r)
            while True:
                reg = reg + (noise * torch.roll(noise, shifts=1, dims=3)).mean() ** 2
                reg = reg + (noise * torch.roll(noise, shifts=1, dims=2)).mean() ** 2
                if noise.shape[2] <= 8:
                    break
                noise = F.avg_pool2d(noise, kernel_size=2)
        out.append(reg)
    return torch.stack(out)


def noise_reg_grad_f64(arena, layout):
    """[K,P] numpy: sum_l 4^-l [2 a_l / N_l (left + right) + 2 b_l / N_l (up + down)] at (y >> l, x >> l), wrapping; zero on W+."""
    arena = _f64(arena).numpy()
    grad = np.zeros_like(arena)
    for k in range(arena.shape[0]):
        for r, o in zip(layout.res, layout.off):
            n = arena[k, o:o + r * r].reshape(r, r)
            g0, lvl = np.zeros([r, r]), 0
            while True:
                cnt = n.size
                a, b = (n * np.roll(n, 1, 1)).mean(), (n * np.roll(n, 1, 0)).mean()
                gl = 2 * a / cnt * (np.roll(n, 1, 1) + np.roll(n, -1, 1)) + 2 * b / cnt * (np.roll(n, 1, 0) + np.roll(n, -1, 0))
                g0 += np.repeat(np.repeat(gl, 1 << lvl, 0), 1 << lvl, 1) / 4.0 ** lvl
                if n.shape[0] <= 8:
                    break
                n = n.reshape(n.shape[0] // 2, 2, n.shape[1] // 2, 2).mean(axis=(1, 3))
                lvl += 1
            grad[k, o:o + r * r] = g0.reshape(-1)
    return grad


# ------------------------------------------------------------------------------------------------
# step, schedule
# ------------------------------------------------------------------------------------------------
def step_f64(arena, grad, m, v, layout, lr, t):
    """(arena, m, v) after one step, numpy float64: Adam (betas 0.9 / 0.999, eps 1e-8, bias-corrected), then per plane
    n -= mean(n); n *= rsqrt(mean(n^2))."""
    arena, grad, m, v = (_f64(x).numpy().copy() for x in (arena, grad, m, v))
    m = 0.9 * m + 0.1 * grad
    v = 0.999 * v + 0.001 * grad * grad
    arena = arena - lr / (1 - 0.9 ** t) * m / (np.sqrt(v) / math.sqrt(1 - 0.999 ** t) + 1e-8)
    for r, o in zip(layout.res, layout.off):
        n = arena[:, o:o + r * r]
        n = n - n.mean(axis=1, keepdims=True)
        arena[:, o:o + r * r] = n / np.sqrt((n * n).mean(axis=1, keepdims=True))
    return arena, m, v


def schedule_f64(step, num_steps, w_std, initial_learning_rate=0.1, initial_noise_factor=0.05, lr_rampdown_length=0.25,
                 lr_rampup_length=0.05, noise_ramp_length=0.75):
    t = step / num_steps
    scale = w_std * initial_noise_factor * max(0.0, 1.0 - t / noise_ramp_length) ** 2
    ramp = min(1.0, (1.0 - t) / lr_rampdown_length)
    ramp = (0.5 - 0.5 * math.cos(ramp * math.pi)) * min(1.0, t / lr_rampup_length)
    return initial_learning_rate * ramp, scale


# ------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------
def line_drawings(r, n, seed=0, width=2):
    """[n,r,r] uint8, 0 = stroke: two to three straight thick lines per drawing on white."""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:r, 0:r]
    out = np.full([n, r, r], 255, np.uint8)
    for i in range(n):
        for _ in range(rs.randint(2, 4)):
            x0, y0, x1, y1 = rs.uniform(0, r, 4)
            d = np.hypot(x1 - x0, y1 - y0) + 1e-6
            t = np.clip(((xx - x0) * (x1 - x0) + (yy - y0) * (y1 - y0)) / d ** 2, 0, 1)
            dist = np.hypot(xx - (x0 + t * (x1 - x0)), yy - (y0 + t * (y1 - y0)))
            out[i][dist <= width] = 0
    return out


def loss_case(r, b, k, seed=0):
    """Inputs of the loss entries: softmax uvs, images in -1..1, a target that EQUALS the image on a region (sign 0), drawing 0 all
    background and -- with b > 1 -- drawing 1 all foreground (eps decides), and exact zeros in uvs on part of sample 0."""
    rs = np.random.RandomState(1000 * r + 10 * b + k + seed)
    uvs = torch.softmax(torch.from_numpy(rs.randn(k * b, 3, r, r).astype(np.float32) * 2), dim=1).numpy()
    img = np.tanh(rs.randn(k * b, 3, r, r)).astype(np.float32)
    target = np.tanh(rs.randn(k * b, 3, r, r)).astype(np.float32)
    target[:, :, : r // 2, : r // 3] = img[:, :, : r // 2, : r // 3]
    geom = (line_drawings(r, b, seed=r + b).astype(np.float32) / 255.0)[:, None]
    geom[0] = 1.0
    if b > 1:
        geom[1] = 0.0
    uvs[0, 2] = 0.0                                                        # s = 0 where g = 1: I = 0; and u = 0 with t = 0 on sample 0
    if b > 1:
        uvs[1, 2] = 0.0                                                    # s = 0 and g = 0: the union is eps alone
    uvs[0, 0, : r // 2] = 0.0
    return dict(uvs=uvs, img=img, target=target, geom=geom, k=k, b=b, r=r, weights=(0.5, 0.5, 50.0))


LOSS_CASES = [(r, b, k) for r in (8, 20, 64) for b in (1, 3) for k in (1, 2)]


def reg_layout():
    return clarity.ArenaLayout(REG_NW, REG_TABLE)


def reg_arena(k=2, seed=3):
    """[k,P] float32 normal values; plane 5 (32 x 32) of row 0 is non-zero only in its first and last row and column, so that only
    products that wrap around contribute at level 0."""
    lo = reg_layout()
    a = np.random.RandomState(seed).randn(k, lo.p).astype(np.float32)
    edge = a[0, lo.off[5]:lo.off[5] + 32 * 32].reshape(32, 32).copy()
    edge[1:-1, 1:-1] = 0.0
    a[0, lo.off[5]:lo.off[5] + 32 * 32] = edge.reshape(-1)
    return a


# ------------------------------------------------------------------------------------------------
# a differentiable generator and an encoder for CPU runs
# ------------------------------------------------------------------------------------------------
class OracleGen:
    """The interface ``clarity.ClarityOptimizer`` asks of a generator, over ``oracle.neube_oracle.OracleGenerator``."""

    def __init__(self, cfg, sd, dtype=torch.float32):
        self.cfg, self.o = cfg, orc.OracleGenerator(cfg, sd, dtype)

    def mapping(self, z, c=None):
        return self.o.mapping(z, c)

    def synthesis(self, ws, geom_feature, noise_mode="const", noise_buffers=None, return_debug_data=False):
        assert noise_mode == "const"
        return self.o.synthesis(ws, geom_feature, return_debug_data=return_debug_data, noise_buffers=noise_buffers)


class StandInEncoder:
    """Geometry features of a drawing without the encoder network: the stroke mask (1 - geom) pooled to each feature resolution, times
    a fixed ramp over the feature's channels."""

    def __init__(self, cfg):
        self.cfg = cfg

    def __call__(self, geom):
        out = []
        for ch, res in zip(self.cfg.geom_feature_channels, self.cfg.geom_feature_resolutions):
            m = F.adaptive_avg_pool2d(1 - geom, res)
            ramp = torch.linspace(-1.0, 1.0, ch, dtype=geom.dtype, device=geom.device).reshape(1, ch, 1, 1)
            out.append(m * ramp * 2.0)
        return out

    encode = __call__


class ReplayDraws(clarity.ClarityDraws):
    """Draws given as arrays: ``init_noise`` [n_brushes, P - nw], ``w_noise`` [steps, n_brushes, num_ws, w_dim], ``drawing_idx`` [steps, B]."""

    def __init__(self, init_noise, w_noise, drawing_idx):
        self.init, self.wn, self.idx = (np.asarray(x) for x in (init_noise, w_noise, drawing_idx))

    def drawings(self, step, batch_size):
        assert self.idx.shape[1] == batch_size
        return torch.from_numpy(self.idx[step].astype(np.int64))

    def initial_noise(self, brush, numel):
        assert self.init.shape[1] == numel
        return torch.from_numpy(self.init[brush].astype(np.float32))

    def w_noise(self, step, brush, shape):
        return torch.from_numpy(self.wn[step, brush].astype(np.float32)).reshape(list(shape))


class DictLibrary:
    """{id: z [1,z_dim]} or {id: w}: the two calls ``ClarityOptimizer`` makes of a library."""

    def __init__(self, zs=None, ws=None):
        self.zs, self.ws = zs or {}, ws or {}

    def get_style_ids(self):
        return sorted(list(self.zs) + list(self.ws))

    def set_style(self, sid, opts):
        if sid in self.zs:
            opts.set_style(torch.as_tensor(self.zs[sid]), style_id=sid)
        else:
            opts.set_style_w(torch.as_tensor(self.ws[sid]), style_id=sid)


def run_statement_loop(gen64, encode, drawings_u8, w_start, draws, num_steps, batch_size, w_std, weights=(0.5, 0.5, 50.0), reg_weight=10.0,
                       lr0=0.1):
    """The loop of opt_clarity_main.py:93-167 for ONE brush in float64, driven by ``draws``: per step (lr, items [3], reg, the smallest
    sqrt(v_hat) of Adam's denominators after the step), and the final arena row.  ``gen64`` an OracleGen of dtype float64."""
    lo = clarity.ArenaLayout.from_config(gen64.cfg)
    arena = np.zeros([1, lo.p])
    arena[0, :lo.nw] = _f64(w_start).numpy().reshape(-1)
    arena[0, lo.nw:] = draws.initial_noise(0, lo.p - lo.nw).numpy()
    m, v, steps = np.zeros_like(arena), np.zeros_like(arena), []
    w0 = _f64(w_start).reshape(1, *lo.w_shape)
    for step in range(num_steps):
        lr, scale = schedule_f64(step, num_steps, w_std, initial_learning_rate=lr0)
        geom = (_f64(drawings_u8[draws.drawings(step, batch_size).numpy()]) / 255.0).unsqueeze(1)
        b = geom.shape[0]
        feats = encode(geom)
        a = torch.from_numpy(arena.copy()).requires_grad_(True)
        nb = lambda t: {n: lo.plane(t, i).reshape(1, 1, lo.res[i], lo.res[i]).expand(b, 1, lo.res[i], lo.res[i]) for i, n in enumerate(lo.names)}
        with torch.no_grad():
            target, _ = gen64.synthesis(w0.expand(b, -1, -1), feats, noise_buffers=nb(a.detach()), return_debug_data=True)
        ws = (lo.w(a) + _f64(draws.w_noise(step, 0, lo.w_shape)).unsqueeze(0) * scale).expand(b, -1, -1)
        img, raw = gen64.synthesis(ws, feats, noise_buffers=nb(a), return_debug_data=True)
        out, _ = loss_f64(raw["uvs"], img, target, geom, 1, weights)
        reg = noise_reg_f64(a, lo)
        (out[0, 3] + reg_weight * reg[0]).backward()
        arena, m, v = step_f64(arena, a.grad.numpy(), m, v, lo, lr, step + 1)
        steps.append((lr, out[0, :3].detach().numpy().copy(), float(reg[0].detach()), float(np.sqrt(v / (1 - 0.999 ** (step + 1))).min())))
    return steps, arena[0]
