"""GPU: the small kernels at the head and tail of every step (csrc/nb_ops.hip) and the device weight packers
(csrc/nb_weight_pack.hip), each through its C entry point on tensors built here, against a float64 restatement
(oracle/neube_oracle.py where it has one) or, for the packers, bit for bit against the package's torch packers.

Layer tables (NbLayerDesc[]) are built with ctypes as networks._Plan does, so that one launch mixes conv layers with
demodulation, a ToRGB entry (n_plain = 9, wsq = NULL) and entries without noise.  Every output lies inside a larger
buffer pre-filled with NaN: rows past the batch, guards around each buffer and a ToRGB entry's dcoefs must stay NaN.

Tolerances: U = 2^-24 is the fp32 unit roundoff.  A sum of L fp32 terms, each formed with a few roundings, is within
(L + k) * U * sum|terms| of the exact sum (k counts the roundings of one term plus the final ones); the bounds below
state L and k for every output and scale by the float64 sum of |terms| of THAT output.  Where an output is a function
of earlier fp32 results (mapping layers, dcoefs from styles, softmax from logits) the bound of the inputs is carried
through the function's derivative, written out at each check.  A dropped or doubled term of a 64-term sum moves an
output by ~1/64 of sum|terms|, about 2^18 / 70 times these bounds."""
import math

import numpy as np
import pytest
import torch

from brushstroke_engine_amd import _lib
from oracle import neube_oracle as orc

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
GUARD = 64                       # NaN floats before and after every output buffer (keeps 16-byte alignment)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


def P(t):
    return None if t is None else t.data_ptr()


def stream():
    return torch.cuda.current_stream().cuda_stream


class Out:
    """An output tensor of `shape` inside a NaN-filled buffer with GUARD elements on either side."""

    def __init__(self, shape, dev, dtype=torch.float32):
        numel = int(np.prod(shape))
        self.buf = torch.full([numel + 2 * GUARD], float("nan"), dtype=dtype, device=dev)
        self.t = self.buf[GUARD:GUARD + numel].view(shape)

    def guards_untouched(self):
        g = torch.cat([self.buf[:GUARD], self.buf[-GUARD:]])
        return bool(torch.isnan(g).all())

    def reset(self):
        self.buf.fill_(float("nan"))


def within(got, want, tol, what):
    """|got - want| <= tol elementwise (float64), and no NaN where a value is expected."""
    got = got.detach().double().cpu() if torch.is_tensor(got) else torch.as_tensor(got, dtype=torch.float64)
    want = want.double().cpu() if torch.is_tensor(want) else torch.as_tensor(want, dtype=torch.float64)
    tol = tol.double().cpu() if torch.is_tensor(tol) else torch.as_tensor(tol, dtype=torch.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert not torch.isnan(got).any(), f"{what}: {int(torch.isnan(got).sum())} outputs never written"
    d = (got - want).abs()
    bad = d > tol
    if bad.any():
        i = int(torch.nonzero(bad.flatten())[0])
        r = float((d / tol.expand_as(d)).max())
        raise AssertionError(f"{what}: {int(bad.sum())} of {d.numel()} outside the bound (worst {r:.3g}x); first at flat index {i}: "
                             f"got {float(got.flatten()[i]):.9g} want {float(want.flatten()[i]):.9g} "
                             f"tol {float(tol.expand_as(d).flatten()[i]):.3g}")


# ---------------------------------------------------------------------------------------------------------------------
# mapping
# ---------------------------------------------------------------------------------------------------------------------

def _mapping_ref(z, fc_w, fc_b, z_dim, w_dim, layers, lr_mul):
    """float64 MappingNetwork (oracle normalize_2nd_moment + fully_connected) and the fp32 error bound of every output.
    normalize_2nd_moment: the mean of z_dim squares (all terms positive: (z_dim + 1) U relative), rsqrtf (2 U), the product
    (1 U) -> e0 = (z_dim / 2 + 4) U |x|.  Layer l (in inputs): sum of in terms cur_i * (w_i * wg) (2 roundings each) plus the
    bias (1) -> (in + 3) U * A_l, A_l = sum|cur_i w_i wg| + |b lr_mul|; lrelu * sqrt2 has slope sqrt2 or 0.2 sqrt2 (sqrt2 where
    the pre-activation lies within its bound of 0) and adds 2 roundings.  The inputs' own errors enter as sum_i (w_i wg) d_i with
    independent rounding errors d_i: carried as the random walk sqrt(sum_i (w_i wg)^2 e_i^2) (the worst case sum |w_i wg| e_i
    grows ~sqrt(in) per layer, which nine layers make useless; FullyConnectedLayer's gain 1 / sqrt(in) keeps the random walk at
    ~e per layer), and the result is taken 4 times for the tail of that walk."""
    x = orc.normalize_2nd_moment(torch.from_numpy(z).double())
    e = (z_dim / 2 + 4) * U * x.abs()
    for l in range(layers):
        w = torch.from_numpy(fc_w[l]).double()
        b = torch.from_numpy(fc_b[l]).double()
        wg = w * (lr_mul / math.sqrt(w.shape[1]))
        pre = orc.fully_connected(x, w, b, lr_multiplier=lr_mul)
        a = x.abs() @ wg.abs().t() + (b * lr_mul).abs()
        e_pre = (w.shape[1] + 3) * U * a + ((e * e) @ (wg * wg).t()).sqrt()
        slope = torch.where(pre.abs() > 4 * e_pre, torch.where(pre > 0, 1.0, 0.2), 1.0).double()
        y = orc.fully_connected(x, w, b, activation="lrelu", lr_multiplier=lr_mul)
        e = math.sqrt(2) * slope * e_pre * (1 + 2 * U) + 2 * U * y.abs()
        x = y
    return x, 4 * e


@pytest.mark.parametrize("z_dim,w_dim,layers", [(64, 64, 8), (64, 64, 9), (1, 16, 2), (40, 40, 2), (512, 512, 3),
                                                (64, 512, 4), (300, 7, 3)])
def test_mapping_vs_float64(dev, z_dim, w_dim, layers):
    """nb_mapping_f32 / nb_mapping_ws_f32: mapping64_kernel (z = w = 64, <= 8 layers, fc_w 16-byte aligned) and mapping_kernel
    (everything else, and the same 64/64 net with fc_w one float off alignment), lr_mul 1 and 0.01, num_ws 1 and 5 (every
    broadcast row), n = 1 and 70; z rows at scales 1e-3 and 1e3 exercise the normalisation."""
    lib = _lib.lib()
    rs = np.random.RandomState(z_dim * 7 + w_dim + layers)
    n_max = 72
    for lr_mul in (1.0, 0.01):
        fc_w = [(rs.randn(w_dim, z_dim if l == 0 else w_dim) / lr_mul).astype(np.float32) for l in range(layers)]
        fc_b = [rs.randn(w_dim).astype(np.float32) for _ in range(layers)]
        z = rs.randn(n_max, z_dim).astype(np.float32)
        z[1] *= 1e-3
        z[2] *= 1e3
        flat = np.concatenate([w.ravel() for w in fc_w])
        for offset in ((0, 1) if (z_dim, w_dim) == (64, 64) else (0,)):
            wbuf = torch.from_numpy(np.concatenate([np.zeros(4, np.float32), flat])).to(dev)
            w_dev = wbuf[4 - offset:4 - offset + flat.size]              # offset 1: fc_w is 4 bytes off a 16-byte boundary
            assert (w_dev.data_ptr() % 16 == 0) == (offset == 0)
            w_dev.copy_(torch.from_numpy(flat).to(dev))
            b_dev = torch.from_numpy(np.concatenate(fc_b)).to(dev)
            z_dev = torch.from_numpy(z).to(dev)
            for n in (1, 70):
                want, tol = _mapping_ref(z[:n], fc_w, fc_b, z_dim, w_dim, layers, lr_mul)
                for num_ws in (1, 5):
                    out = Out([n_max, num_ws, w_dim], dev)
                    if num_ws == 1:
                        rc = lib.nb_mapping_f32(P(z_dev), P(w_dev), P(b_dev), P(out.t), n, z_dim, w_dim, layers, lr_mul, stream())
                    else:
                        rc = lib.nb_mapping_ws_f32(P(z_dev), P(w_dev), P(b_dev), P(out.t), n, z_dim, w_dim, layers, lr_mul, num_ws,
                                                   stream())
                    _lib.check(rc, "mapping")
                    torch.cuda.synchronize()
                    what = f"mapping z{z_dim} w{w_dim} L{layers} lr{lr_mul} off{offset} n{n} ws{num_ws}"
                    for k in range(num_ws):
                        within(out.t[:n, k], want, tol, f"{what} row {k}")
                    assert torch.isnan(out.t[n:]).all() and out.guards_untouched(), f"{what}: stray write"


# ---------------------------------------------------------------------------------------------------------------------
# styles, demodulation, noise: one NbLayerDesc table
# ---------------------------------------------------------------------------------------------------------------------

class Table:
    """NbLayerDesc[] on the device with its weights and NaN-guarded outputs.  spec: dict(c_aff, c_out, n_plain=0, wsq=True,
    res=0 (no noise), w_index)."""

    def __init__(self, specs, w_dim, n_max, dev, seed):
        rs = np.random.RandomState(seed)
        self.specs, self.w_dim, self.n_max, self.dev = specs, w_dim, n_max, dev
        self.keep, self.out = [], []
        descs = (_lib.NbLayerDesc * len(specs))()
        for i, s in enumerate(specs):
            c_aff, c_out, n_plain = s["c_aff"], s["c_out"], s.get("n_plain", 0)
            c_in = c_aff - n_plain
            t = {"aw": rs.randn(c_aff, w_dim).astype(np.float32), "ab": rs.randn(c_aff).astype(np.float32),
                 "wsq": (rs.rand(c_in, c_out) * 2).astype(np.float32) if s.get("wsq", True) else None,
                 "scale": np.float32(1 / math.sqrt(c_in)) if n_plain else np.float32(1.0)}
            o = {"styles": Out([n_max, c_aff], dev), "dcoefs": Out([n_max, c_out], dev)}
            d = descs[i]
            dv = {k: torch.from_numpy(v).to(dev) for k, v in t.items() if isinstance(v, np.ndarray) and v.ndim}
            d.affine_w, d.affine_b = P(dv["aw"]), P(dv["ab"])
            d.wsq = P(dv["wsq"]) if t["wsq"] is not None else 0
            d.styles, d.dcoefs = P(o["styles"].t), P(o["dcoefs"].t)       # (a ToRGB entry's dcoefs must stay NaN)
            r = s.get("res", 0)
            if r:
                t["nc"] = rs.randn(r, r).astype(np.float32)
                t["lin"] = torch.linspace(0, 1, r, dtype=torch.float32).numpy()
                t["strength"] = np.array([rs.randn()], np.float32)
                for k in ("nc", "lin", "strength"):
                    dv[k] = torch.from_numpy(t[k]).to(dev)
                o["noise"] = Out([n_max, r, r], dev)
                d.noise_const, d.noise_lin, d.noise_strength = P(dv["nc"]), P(dv["lin"]), P(dv["strength"])
                d.noise_out = P(o["noise"].t)
            d.c_aff, d.n_plain, d.c_out, d.w_index, d.res = c_aff, n_plain, c_out, s["w_index"], r
            d.style_scale = float(t["scale"])
            self.keep.append((t, dv))
            self.out.append(o)
        self.dev_table = torch.from_numpy(np.frombuffer(bytes(descs), dtype=np.uint8).copy()).to(dev)

    def reset(self):
        for o in self.out:
            for b in o.values():
                b.reset()

    def styles_ref(self, ws, i):
        """float64 affine (FullyConnectedLayer, weight_gain 1/sqrt(w_dim)) * style_scale past n_plain, and its bound:
        w_dim terms ws_i * (a_i * wg) (2 roundings each), the bias and the scale -> (w_dim + 4) U (sum|terms| + |b|) |scale|."""
        t, s = self.keep[i][0], self.specs[i]
        w = torch.from_numpy(ws[:, s["w_index"]]).double()
        a = torch.from_numpy(t["aw"]).double()
        b = torch.from_numpy(t["ab"]).double()
        y = orc.fully_connected(w, a, b)
        absum = w.abs() @ a.abs().t() / math.sqrt(self.w_dim) + b.abs()
        sc = torch.ones(y.shape[1], dtype=torch.float64)
        sc[s.get("n_plain", 0):] = float(t["scale"])
        return y * sc, (self.w_dim + 4) * U * absum * sc

    def dcoefs_ref(self, ws, i):
        """d = rsqrt(sum_i s_i^2 wsq_io + 1e-8) in float64 from the float64 styles.  The fp32 sum: c_in terms s_i * s_i * wsq
        (2 roundings each) plus 1e-8 -> (c_in + 3) U Q, Q = sum s^2 wsq; the styles' own bound e_s adds sum 2 |s| e_s wsq.
        rsqrtf adds 2 U, and d = Q^-1/2 turns a relative error r of Q into r / 2."""
        s_ref, e_s = self.styles_ref(ws, i)
        n_plain = self.specs[i].get("n_plain", 0)
        s, e = s_ref[:, n_plain:], e_s[:, n_plain:]
        wsq = torch.from_numpy(self.keep[i][0]["wsq"]).double()
        q = (s * s) @ wsq + 1e-8
        dq = (self.specs[i]["c_aff"] - n_plain + 3) * U * q + (2 * s.abs() * e + e * e) @ wsq
        d = q.rsqrt()
        return d, d * (0.5 * dq / q + 4 * U)


def _check_styles(tab, ws, n, what, dcoefs=True):
    for i, s in enumerate(tab.specs):
        o = tab.out[i]
        want, tol = tab.styles_ref(ws[:n], i)
        within(o["styles"].t[:n], want, tol, f"{what} layer {i} styles")
        assert torch.isnan(o["styles"].t[n:]).all() and o["styles"].guards_untouched(), f"{what} layer {i}: stray styles write"
        if dcoefs and s.get("wsq", True):
            want, tol = tab.dcoefs_ref(ws[:n], i)
            within(o["dcoefs"].t[:n], want, tol, f"{what} layer {i} dcoefs")
            assert torch.isnan(o["dcoefs"].t[n:]).all() and o["dcoefs"].guards_untouched(), f"{what} layer {i}: stray dcoefs write"
        else:
            assert torch.isnan(o["dcoefs"].buf).all(), f"{what} layer {i}: dcoefs written for an entry without demodulation"


def _styles_specs(num_ws, big):
    """c_out 4 / 12 / 20 (empty and partial per-part slices), 1024 (the float4 path at ng = 64), 1028 and 1500 (the plain loop,
    ng > 64); c_aff 3, 9 + 3 (ToRGB), 1024; with `big` also c_aff 1025 and 1500 and a ToRGB of 1024 + 9 (past the LDS array)."""
    sp = [dict(c_aff=3, c_out=4), dict(c_aff=12, n_plain=9, c_out=3, wsq=False), dict(c_aff=1024, c_out=20),
          dict(c_aff=300, c_out=12), dict(c_aff=64, c_out=1024), dict(c_aff=200, c_out=1028), dict(c_aff=1024, c_out=1500)]
    if big:
        sp += [dict(c_aff=1025, c_out=1028), dict(c_aff=1500, c_out=1500), dict(c_aff=1033, n_plain=9, c_out=3, wsq=False),
               dict(c_aff=1100, c_out=7)]
    for i, s in enumerate(sp):
        s["w_index"] = (3 * i + 1) % num_ws                    # != the layer index
    return sp


@pytest.mark.parametrize("w_dim", [16, 48, 512, 40])
def test_styles_and_dcoefs_vs_float64(dev, w_dim):
    """nb_styles_f32 (every table, c_aff up to 1500: the squares past its 1024-entry LDS array come from the styles it wrote)
    and nb_styles_fast_f32 (w_dim % 16 == 0, c_aff <= 1024, c_out % 4 == 0) against float64, n = 1 and 70 of 72 rows."""
    lib = _lib.lib()
    num_ws, n_max = 5, 72
    rs = np.random.RandomState(w_dim)
    ws = rs.randn(n_max, num_ws, w_dim).astype(np.float32)
    ws_dev = torch.from_numpy(ws).to(dev)
    kinds = [("slow", True)] + ([("fast", False)] if w_dim % 16 == 0 else [])
    for kind, big in kinds:
        specs = _styles_specs(num_ws, big)
        if kind == "slow":
            specs.append(dict(c_aff=33, c_out=5, w_index=2))       # (c_out % 4 != 0: the plain kernel only)
        tab = Table(specs, w_dim, n_max, dev, seed=w_dim + 1)
        fn = lib.nb_styles_f32 if kind == "slow" else lib.nb_styles_fast_f32
        for n in (1, 70):
            tab.reset()
            _lib.check(fn(P(tab.dev_table), len(specs), P(ws_dev), num_ws, w_dim, n, stream()), kind)
            torch.cuda.synchronize()
            _check_styles(tab, ws, n, f"styles {kind} w_dim {w_dim} n {n}")


def test_styles_noise_matches_fast_and_noise(dev):
    """nb_styles_noise_f32 = nb_styles_fast_f32 (styles, dcoefs) + nb_noise_f32 (noise images), bit for bit, with positions and
    with norm_pos; layers with and without noise in one table."""
    lib = _lib.lib()
    num_ws, w_dim, n_max, R = 4, 64, 10, 256
    specs = [dict(c_aff=3, c_out=4, res=4), dict(c_aff=64, c_out=20, res=8), dict(c_aff=12, n_plain=9, c_out=3, wsq=False),
             dict(c_aff=300, c_out=1028, res=16), dict(c_aff=1024, c_out=64), dict(c_aff=128, c_out=128, res=64)]
    for i, s in enumerate(specs):
        s["w_index"] = (i + 2) % num_ws
    tab = Table(specs, w_dim, n_max, dev, seed=3)
    rs = np.random.RandomState(4)
    ws = torch.from_numpy(rs.randn(n_max, num_ws, w_dim).astype(np.float32)).to(dev)
    pos = torch.from_numpy(np.array([[-3, 255], [256, 2 ** 40], [-2 ** 40, 7], [5, -1], [100, 31], [0, 0], [254, 1], [13, 200]],
                                    np.int64)).to(dev)
    npos = Out([8, 2], dev)
    _lib.check(lib.nb_norm_positions_f32(P(pos), R, P(npos.t), 8, stream()), "norm_positions")
    for n in (1, 8):
        for form in ("positions", "norm_pos"):
            ip, fp = (pos, None) if form == "positions" else (None, npos.t)
            tab.reset()
            _lib.check(lib.nb_styles_noise_f32(P(tab.dev_table), len(specs), P(ws), num_ws, w_dim, P(fp), P(ip), R, n, stream()),
                       "styles_noise")
            fused = [{k: b.buf.clone() for k, b in o.items()} for o in tab.out]
            tab.reset()
            _lib.check(lib.nb_styles_fast_f32(P(tab.dev_table), len(specs), P(ws), num_ws, w_dim, n, stream()), "styles_fast")
            _lib.check(lib.nb_noise_f32(P(tab.dev_table), len(specs), 64, P(fp), P(ip), R, n, stream()), "noise")
            torch.cuda.synchronize()
            for i, o in enumerate(tab.out):
                for k, b in o.items():
                    assert torch.equal(fused[i][k].view(torch.int32), b.buf.view(torch.int32)), (n, form, i, k)
            _check_styles(tab, ws.cpu().numpy(), n, f"styles_noise n {n} {form}")


@pytest.mark.parametrize("c_in,c_out", [(1, 1), (2000, 700), (33, 257), (1000, 3), (64, 64), (7, 513)])
def test_demod_coefs_vs_float64(dev, c_in, c_out):
    """nb_demod_coefs_f32: d = rsqrt(sum_i s_i^2 wsq_io + 1e-8); fp32 sum of c_in terms (s * s) * wsq (2 roundings each) and the
    1e-8 -> (c_in + 3) U Q relative to Q, rsqrtf 2 U, halved by the square root: d * ((c_in + 3) U / 2 + 4 U)."""
    lib = _lib.lib()
    rs = np.random.RandomState(c_in + c_out)
    n, n_max = 3, 4
    s = rs.randn(n, c_in).astype(np.float32)
    wsq = (rs.rand(c_in, c_out) * 2).astype(np.float32)
    out = Out([n_max, c_out], dev)
    s_dev, wsq_dev = torch.from_numpy(s).to(dev), torch.from_numpy(wsq).to(dev)
    _lib.check(lib.nb_demod_coefs_f32(P(s_dev), P(wsq_dev), P(out.t), n, c_in, c_out, stream()), "demod")
    torch.cuda.synchronize()
    sd, wd = torch.from_numpy(s).double(), torch.from_numpy(wsq).double()
    d = ((sd * sd) @ wd + 1e-8).rsqrt()
    within(out.t[:n], d, d * ((c_in + 3) * U / 2 + 4 * U), f"demod {c_in}x{c_out}")
    assert torch.isnan(out.t[n:]).all() and out.guards_untouched()


# ---------------------------------------------------------------------------------------------------------------------
# noise
# ---------------------------------------------------------------------------------------------------------------------

def test_noise_vs_float64(dev):
    """nb_noise_f32 against oracle shifted_const_noise (float32 sample coordinates, float64 interpolation): res 4 ... 256 in one
    table with max_res 256 (several 32 x 32 tiles per block for res 64 / 256, one partial tile for the small layers), an entry
    without noise, positions negative, R - 1, R and +-2^40.  The fp32 value is 4 taps * (wx * wy) (2 roundings each), their sum
    (3) and the strength (1): 9 U * strength * sum|tap wx wy|.  nb_norm_positions_f32 = the reference's (p mod R) / (R - 1) in
    float32, bit for bit, and the norm_pos form of the launch equals the positions form bit for bit.  Without positions only
    sample 0 is written: noise_const * strength."""
    lib = _lib.lib()
    R, n, n_max = 256, 6, 8
    res = [4, 8, 16, 64, 256]
    specs = [dict(c_aff=3, c_out=4, res=r, w_index=0) for r in res[:2]] + [dict(c_aff=3, c_out=4, w_index=0)] + \
            [dict(c_aff=3, c_out=4, res=r, w_index=0) for r in res[2:]]
    tab = Table(specs, 16, n_max, dev, seed=9)
    pos_np = np.array([[-1, -300], [R - 1, R], [R, R - 1], [2 ** 40, -2 ** 40], [-2 ** 40 - 5, 2 ** 40 + 3], [17, 129]], np.int64)
    pos = torch.from_numpy(pos_np).to(dev)
    npos = Out([n_max, 2], dev)
    _lib.check(lib.nb_norm_positions_f32(P(pos), R, P(npos.t), n, stream()), "norm_positions")
    torch.cuda.synchronize()
    want_np = (torch.remainder(torch.from_numpy(pos_np), R).to(torch.float32) / torch.tensor(R - 1, dtype=torch.float32))
    assert torch.equal(npos.t[:n].cpu(), want_np) and torch.isnan(npos.t[n:]).all() and npos.guards_untouched()
    got = {}
    for form in ("positions", "norm_pos"):
        tab.reset()
        ip, fp = (pos, None) if form == "positions" else (None, npos.t)
        _lib.check(lib.nb_noise_f32(P(tab.dev_table), len(specs), R, P(fp), P(ip), R, n, stream()), "noise")
        torch.cuda.synchronize()
        got[form] = [o["noise"].buf.clone() if "noise" in o else None for o in tab.out]
        for i, s in enumerate(specs):
            o = tab.out[i]
            if "noise" not in o:
                continue
            t = tab.keep[i][0]
            r = s["res"]
            lin = torch.from_numpy(t["lin"])
            grid = torch.stack([lin[:, None].expand(r, r), lin[None, :].expand(r, r)], dim=-1)      # grid[i, j] = (lin[i], lin[j])
            nc = torch.from_numpy(t["nc"]).double()
            st = float(t["strength"][0])
            want = orc.shifted_const_noise(nc, grid, want_np)[:, 0] * st
            absum = orc.shifted_const_noise(nc.abs(), grid, want_np)[:, 0] * abs(st)
            within(o["noise"].t[:n], want, 9 * U * absum, f"noise {form} res {r}")
            assert torch.isnan(o["noise"].t[n:]).all() and o["noise"].guards_untouched(), f"noise {form} res {r}: stray write"
            assert torch.isnan(o["styles"].buf).all() and torch.isnan(o["dcoefs"].buf).all()
    for a, b in zip(got["positions"], got["norm_pos"]):
        assert a is None or torch.equal(a.view(torch.int32), b.view(torch.int32))
    tab.reset()
    _lib.check(lib.nb_noise_f32(P(tab.dev_table), len(specs), R, None, None, R, n, stream()), "noise const")
    torch.cuda.synchronize()
    for i, o in enumerate(tab.out):
        if "noise" in o:
            t = tab.keep[i][0]
            want = torch.from_numpy(t["nc"]) * torch.from_numpy(t["strength"])[0]
            assert torch.equal(o["noise"].t[0].cpu(), want), f"const noise layer {i}"
            assert torch.isnan(o["noise"].t[1:]).all() and o["noise"].guards_untouched(), f"const noise layer {i}: samples > 0 written"


# ---------------------------------------------------------------------------------------------------------------------
# ToRGB triad + compositing
# ---------------------------------------------------------------------------------------------------------------------

OUTS = ("logits", "uvs", "img", "colors_out", "rgba_f32", "rgba_u8")


def _torgb_run(lib, x, st, stride, w, b, cb, clamp, uc, sf, mode, n, c, hw, dev, drop=None):
    o = {"logits": Out([n, 3, hw], dev), "uvs": Out([n, 3, hw], dev), "img": Out([n, 3, hw], dev), "colors_out": Out([n, 9], dev),
         "rgba_f32": Out([n, 4, hw], dev)}
    u8 = torch.full([n * hw * 4 + 2 * GUARD], 0xA5, dtype=torch.uint8, device=dev)
    ptr = {k: P(v.t) for k, v in o.items()}
    ptr["rgba_u8"] = u8.data_ptr() + GUARD
    if drop:
        ptr[drop] = None
    _lib.check(lib.nb_torgb_triad_f32(P(x), P(st), stride, P(w), P(b), P(cb), clamp, ptr["logits"], ptr["uvs"], ptr["img"],
                                      ptr["colors_out"], P(uc), P(sf), mode, ptr["rgba_f32"], ptr["rgba_u8"], n, c, hw, stream()),
               "torgb_triad")
    torch.cuda.synchronize()
    return o, u8


def _torgb_ref(x, st, w, b, cb, clamp, uc, sf, mode, c, x_err=0.0):
    """float64 ToRGBColorTriadLayer arithmetic (OracleGenerator.torgb after its affine) + triad_composite, with bounds.
    x_err (default 0: x is the kernel's own input) = bound of the error of every x the kernel sees (a fused producer's output
    against the float64 x given here); it enters the logits as x_err * sum_c |w_c s_c| and is carried on from there.
    logits: c terms x * (w * s) (2 roundings each; fmaf accumulation in 8 partial sums, then 7 adds) + bias ->
    E = (c + 10) U (sum|x w s| + |b|); the clamp is 1-Lipschitz.  softmax: du_k = u_k (dl_k - sum_j u_j dl_j), so
    |du_k| <= 2 E_max u_k (1 - u_k), plus expf / 1/x / products: 16 U.  img_ch = sum_k u_k col_k: sum |du_k| |col_k| + 12 U sum
    u_k |col_k| (tanhf: 4 U).  _map_style_s: s' = min(sf s, 1) moves by sf |ds| + 2 U; u' = (1 - s') r with r = u / (u + v) =
    1 / (1 + e^(l1 - l0)), |dr| <= 2 E r (1 - r) + 8 U; |du'| <= |ds'| r + (1 - s') |dr| + 8 U (|ds'| from the extremes of s
    within its bound).  rgba_ch = sum_k m_k c01_k likewise, c01 = (col + 1) / 2 within 4 U absolute; alpha = u' + v' (render
    mode 0) or exactly 1.  Pixels where s' = min(sf s, 1) within its bound can fall on either side of 1 - s' <= 1e-6 are
    returned in `ambiguous` (the caller skips them in the RGBA checks)."""
    xd = x.double()
    s = st[:, 9:9 + c].double()
    wm = w.double()[None] * s[:, None, :]                                   # [n, 3, c]
    pre = torch.einsum("noc,nch->noh", wm, xd)
    A = torch.einsum("noc,nch->noh", wm.abs(), xd.abs()) + b.double().abs()[None, :, None]
    logits = orc.bias_act(pre, b.double(), clamp=clamp if clamp >= 0 else None)
    E = (c + 10) * U * A + x_err * wm.abs().sum(dim=2)[:, :, None]
    Emax = E.max(dim=1, keepdim=True).values
    uvs = torch.softmax(logits, dim=1)
    tol_u = 2 * Emax * uvs * (1 - uvs) + 16 * U
    colors = torch.tanh(st[:, :9].double() + cb.double()).reshape(-1, 3, 3)
    img = torch.sum(uvs.unsqueeze(1) * colors.unsqueeze(-1), dim=2)
    tol_img = torch.sum(tol_u.unsqueeze(1) * colors.abs().unsqueeze(-1) + 12 * U * (uvs.unsqueeze(1) * colors.abs().unsqueeze(-1)),
                        dim=2) + 4 * U
    sfd = None if sf is None else sf.double()[:, None, None]
    sf4 = None if sf is None else sf.double()[:, None, None, None]              # (the oracle's images are [n, ch, h, w]: h = 1)
    rgba = orc.triad_composite(uvs.unsqueeze(2), colors, "clear" if mode == 0 else "full",
                               user_colors=None if uc is None else uc.double().reshape(-1, 3, 3), sfactor=sf4)[:, :, 0]
    col01 = (colors + 1) / 2
    if uc is not None:
        ucd = uc.double().reshape(-1, 3, 3)
        col01 = torch.where(torch.isnan(ucd), col01, ucd)
    if sf is None:
        m, tol_m = uvs, tol_u
        ambiguous = torch.zeros_like(uvs[:, 0], dtype=torch.bool)
    else:
        m = orc.map_style_s(sf4, uvs.unsqueeze(2))[:, :, 0]
        sp = torch.clamp(sfd[:, 0] * uvs[:, 2], max=1.0)
        sp_hi = torch.clamp(sfd[:, 0] * (uvs[:, 2] + tol_u[:, 2]), max=1.0)      # s' of the extremes of s
        sp_lo = torch.clamp(sfd[:, 0] * (uvs[:, 2] - tol_u[:, 2]).clamp(min=0), max=1.0)
        d_sp = (sp_hi - sp_lo) + 2 * U
        delta = 1 - sp
        r = uvs[:, 0] / (uvs[:, 0] + uvs[:, 1])
        dr = 2 * Emax[:, 0] * r * (1 - r) + 8 * U
        f0 = (delta <= 1e-6).unsqueeze(1)
        t_uv = torch.stack([d_sp * r + delta * dr, d_sp * (1 - r) + delta * dr], 1) + 8 * U
        tol_m = torch.cat([torch.where(f0, torch.zeros_like(t_uv), t_uv), d_sp.unsqueeze(1)], 1)
        ambiguous = (1 - sp_hi <= 1e-6 + 4 * U) & (1 - sp_lo > 1e-6 - 4 * U)    # the f = 0 branch may go either way
    tol_rgb = torch.sum(tol_m.unsqueeze(1) * col01.abs().unsqueeze(-1) + 12 * U * m.unsqueeze(1) * col01.abs().unsqueeze(-1), dim=2) \
        + 4 * U * m.sum(1, keepdim=True)                                      # (tanhf's absolute 4 U carries into (col + 1) / 2)
    tol_a = tol_m[:, 0:1] + tol_m[:, 1:2] + 4 * U if mode == 0 else torch.zeros_like(tol_m[:, :1])
    return dict(logits=(logits, E), uvs=(uvs, tol_u), img=(img, tol_img), colors_out=(colors.reshape(-1, 9), U * (st[:, :9].double() + cb.double()).abs() + 4 * U),
                rgba_f32=(rgba, torch.cat([tol_rgb, tol_a], 1))), ambiguous


CASES = [  # (c, hw, x offset in floats, n, clamp, render mode, sfactor kind, user colors)
    (1, 16, 0, 2, -1.0, 0, None, False),
    (7, 37, 0, 3, 0.5, 1, "mixed", True),          # hw % 4 != 0: torgb_triad_kernel<1>
    (8, 2048, 1, 2, 256.0, 0, "mixed", True),      # x one float off alignment: <1>, 8 blocks along x
    (100, 4096, 0, 3, 256.0, 0, "mixed", False),   # <4>, 4 blocks along x
    (512, 1028, 0, 2, -1.0, 1, None, True),
    (100, 37, 1, 70, 0.5, 0, "mixed", True),
]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_torgb_triad_vs_float64(dev, case):
    """nb_torgb_triad_f32 against the float64 torgb + triad_composite arithmetic (bounds in _torgb_ref): <4> and <1>, c 1 ... 512,
    clamp -1 / 0.5 / 256, render modes 0 and 1, user colors partly NaN, sfactor below 1, above 1, one that puts a pixel at
    1 - s' ~ 5e-4 and one large enough that s' = 1 (f = 0), colors_out of every sample with several blocks along x.
    rgba_u8 = trunc(clamp(rgba_f32 * 255)) of the kernel's own rgba_f32 bit for bit, and within one step of the float64
    reference (truncation is discontinuous).  Then every output pointer is left NULL in turn: the others do not change."""
    lib = _lib.lib()
    c, hw, xoff, n, clamp, mode, sfk, ucol = CASES[case]
    rs = np.random.RandomState(100 + case)
    stride = c + 9 + 3
    xbuf = torch.from_numpy((rs.randn(n * c * hw + 4) * (2 / math.sqrt(c))).astype(np.float32)).to(dev)   # (logits ~ N(0, 9))
    x = xbuf[xoff:xoff + n * c * hw]
    st = torch.from_numpy((rs.randn(n, stride) * 1.5).astype(np.float32)).to(dev)
    w = torch.from_numpy(rs.randn(3, c).astype(np.float32)).to(dev)
    b = torch.from_numpy(rs.randn(3).astype(np.float32)).to(dev)
    cb = torch.from_numpy(rs.randn(9).astype(np.float32)).to(dev)
    uc = None
    if ucol:
        u = rs.rand(n, 9).astype(np.float32)
        u[rs.rand(n, 9) < 0.5] = np.nan
        uc = torch.from_numpy(u).to(dev)
    sf = None
    if sfk:
        v = np.array([0.5, 1.7, 1e9] + [rs.choice([0.3, 1.5, 3.0, 1e6]) for _ in range(n - 3)], np.float32)[:n]
        sf = torch.from_numpy(v).to(dev)
    xv = x.view(n, c, hw)
    if sf is not None and n > 3:
        # sample 3: sfactor that leaves 1 - s' ~ 5e-4 at pixel 0 (the f != 0 branch with a small delta)
        want0, _ = _torgb_ref(xv[3:4, :, :1].cpu(), st[3:4].cpu(), w.cpu(), b.cpu(), cb.cpu(), clamp, None, None, mode, c)
        sv = sf.cpu().numpy()
        sv[3] = np.float32((1 - 5e-4) / float(want0["uvs"][0][0, 2, 0]))
        sf = torch.from_numpy(sv).to(dev)
    o, u8 = _torgb_run(lib, x, st, stride, w, b, cb, clamp, uc, sf, mode, n, c, hw, dev)
    ref, amb = _torgb_ref(xv.cpu(), st.cpu(), w.cpu(), b.cpu(), cb.cpu(), clamp, None if uc is None else uc.cpu(),
                          None if sf is None else sf.cpu(), mode, c)
    assert float(amb.double().mean()) < 0.1, "too many pixels at the f = 0 threshold"
    what = f"torgb c{c} hw{hw} off{xoff} n{n} clamp{clamp} mode{mode}"
    for k in ("logits", "uvs", "img", "colors_out", "rgba_f32"):
        got = o[k].t
        want, tol = ref[k]
        if k == "rgba_f32":
            keep = ~amb.unsqueeze(1).expand_as(want)
            got, want, tol = got.cpu()[keep], want[keep], tol.expand_as(want)[keep]
        within(got, want, tol, f"{what} {k}")
        assert o[k].guards_untouched(), f"{what} {k}: stray write"
    body = u8[GUARD:GUARD + n * hw * 4].view(n, hw, 4)
    assert bool((u8[:GUARD] == 0xA5).all() and (u8[GUARD + n * hw * 4:] == 0xA5).all()), f"{what}: stray rgba_u8 write"
    mine = (o["rgba_f32"].t * 255).clamp(0, 255).to(torch.uint8).permute(0, 2, 1)
    assert torch.equal(body, mine), f"{what}: rgba_u8 != trunc(clamp(rgba_f32 * 255))"
    want8 = (ref["rgba_f32"][0] * 255).clamp(0, 255).floor().permute(0, 2, 1)
    du = (body.cpu().double() - want8).abs()
    du[amb.unsqueeze(-1).expand_as(du)] = 0
    assert float(du.max()) <= 1, f"{what}: rgba_u8 more than one step from float64"
    if case == 2:
        for drop in OUTS:
            o2, u82 = _torgb_run(lib, x, st, stride, w, b, cb, clamp, uc, sf, mode, n, c, hw, dev, drop=drop)
            for k in OUTS[:5]:
                if k == drop:
                    assert torch.isnan(o2[k].buf).all(), (drop, k)
                else:
                    assert torch.equal(o2[k].buf.view(torch.int32), o[k].buf.view(torch.int32)), (drop, k)
            assert torch.equal(u82, torch.full_like(u8, 0xA5) if drop == "rgba_u8" else u8), drop


# ---------------------------------------------------------------------------------------------------------------------
# blend
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nf,na", [(1, 1), (1, 3), (3, 1), (3, 3)])
def test_blend_vs_float64(dev, nf, na):
    """nb_blend_f32 (oracle blend) with features / alpha broadcast or per sample, 3 x 7 x 99999 = 2.1e6 elements: more than the
    8192 x 256 the grid covers (grid-stride loop), c * hw = 699993 not a multiple of 256.  y = a f + (1 - a) x: 3 roundings on
    a f + (1 - a) x and 1 on 1 - a -> 4 U (|a f| + |1 - a| |x|) + U |x|."""
    lib = _lib.lib()
    n, c, hw = 3, 7, 99999
    assert n * c * hw > 8192 * 256 and (c * hw) % 256
    g = torch.Generator().manual_seed(nf * 10 + na)
    f = torch.randn(nf, c, hw, generator=g)
    a = torch.rand(na, 1, hw, generator=g) * 1.4 - 0.2
    x = torch.randn(n, c, hw, generator=g)
    out = Out([n, c, hw], dev)
    f_dev, a_dev, x_dev = f.to(dev), a.to(dev), x.to(dev)
    _lib.check(lib.nb_blend_f32(P(f_dev), nf, P(a_dev), na, P(x_dev), P(out.t), n, c, hw, stream()), "blend")
    torch.cuda.synchronize()
    fd, ad, xd = f.double(), a.double(), x.double()
    want = orc.blend(fd, ad, xd)
    within(out.t, want.expand(n, c, hw), 4 * U * ((ad * fd).abs() + (1 - ad).abs() * xd.abs()) + U * xd.abs(), f"blend nf{nf} na{na}")
    assert out.guards_untouched()


# ---------------------------------------------------------------------------------------------------------------------
# device weight packers
# ---------------------------------------------------------------------------------------------------------------------

def _bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()])


def _packed(shape, dtype, dev):
    """NaN-filled output with guards (padding the packer must zero, stray writes past the end)."""
    return Out(shape, dev, dtype)


@pytest.mark.parametrize("c_in", [1, 5, 16, 36, 144, 300])
def test_device_packers_match_torch_packers(dev, c_in):
    """nb_pack_conv_weight_dev (wpk, wsq), nb_pack_conv_weight_h3f8_dev, nb_pack_conv_weight_h3_up2_dev (also through
    native.pack_weights_dev) and nb_pack_conv_weight_h3_dev at co_align 64 / 128 and transpose_flip 0 / 1, bit for bit equal to
    ops.pack_conv_weight, w.square().sum([2, 3]).t(), ops.pack_conv_weight_h3f8, ops.pack_conv_weight_h3_up2_phases and
    ops.pack_conv_weight_h3 of the described weight padded to co_align, on the same device.  Outputs start as NaN: every
    padding lane must be written as zero, and nothing past the end."""
    from brushstroke_engine_amd import native, ops
    lib = _lib.lib()
    f = ops.setup_filter((1, 3, 3, 1), device=dev)
    for c_out in (1, 3, 33, 64, 130):
        g = torch.Generator().manual_seed(c_in * 1000 + c_out)
        w = torch.randn(c_out, c_in, 3, 3, generator=g).to(dev)
        what = f"c_in {c_in} c_out {c_out}"
        nch, op64 = (c_in + 15) // 16, (c_out + 63) // 64 * 64
        # wpk / wsq
        wpk = _packed([(c_in + 7) // 8 * 8, 9, (c_out + 31) // 32 * 32], torch.float32, dev)
        wsq = _packed([c_in, c_out], torch.float32, dev)
        _lib.check(lib.nb_pack_conv_weight_dev(P(w), c_out, c_in, P(wpk.t), P(wsq.t), stream()), "pack_conv_weight_dev")
        want_wpk, want_wsq = ops.pack_conv_weight(w)
        torch.cuda.synchronize()
        assert torch.equal(_bits(wpk.t), _bits(want_wpk)) and wpk.guards_untouched(), f"{what}: wpk"
        assert torch.equal(_bits(wsq.t), _bits(w.square().sum([2, 3]).t())) and wsq.guards_untouched(), f"{what}: wsq"
        assert torch.equal(_bits(want_wsq), _bits(w.square().sum([2, 3]).t()))
        # f8
        f8 = _packed([nch, 3, 3, 2, 2, op64, 8], torch.float16, dev)
        _lib.check(lib.nb_pack_conv_weight_h3f8_dev(P(w), c_out, c_in, P(f8.t), stream()), "pack_conv_weight_h3f8_dev")
        want = ops.pack_conv_weight_h3f8(w)
        torch.cuda.synchronize()
        assert torch.equal(_bits(f8.t), _bits(want)) and f8.guards_untouched(), f"{what}: f8"
        # h3_up2 (four FIR-folded phase kernels)
        up2 = _packed([4, nch, 3, 3, 2, 2, op64, 8], torch.float16, dev)
        _lib.check(lib.nb_pack_conv_weight_h3_up2_dev(P(w), P(f), c_out, c_in, P(up2.t), stream()), "pack_conv_weight_h3_up2_dev")
        want = ops.pack_conv_weight_h3_up2_phases(w, f)
        torch.cuda.synchronize()
        assert torch.equal(_bits(up2.t), _bits(want)) and up2.guards_untouched(), f"{what}: h3_up2"
        # the same through the package's entry
        got_wpk, got_wsq = native.pack_weights_dev(w, "wpk")
        assert torch.equal(_bits(got_wpk), _bits(want_wpk)) and torch.equal(_bits(got_wsq), _bits(want_wsq)), what
        assert torch.equal(_bits(native.pack_weights_dev(w, "f8")), _bits(f8.t)), what
        assert torch.equal(_bits(native.pack_weights_dev(w, "h3_up2", f)), _bits(up2.t)), what
        # h3 at co_align 64 / 128, transpose_flip 0 / 1
        for co_align in (64, 128):
            for tf in (0, 1):
                wt = w.transpose(0, 1).flip([2, 3]) if tf else w                  # the weight that gets packed
                o_, i_ = wt.shape[:2]
                op = (o_ + co_align - 1) // co_align * co_align
                out = _packed([(i_ + 15) // 16, 3, 3, 2, 2, op, 8], torch.float16, dev)
                _lib.check(lib.nb_pack_conv_weight_h3_dev(P(w), o_, i_, co_align, tf, P(out.t), stream()), "pack_conv_weight_h3_dev")
                wpad = torch.zeros(op, i_, 3, 3, device=dev)
                wpad[:o_] = wt
                want = ops.pack_conv_weight_h3(wpad)
                torch.cuda.synchronize()
                assert torch.equal(_bits(out.t), _bits(want)) and out.guards_untouched(), f"{what}: h3 co_align {co_align} tf {tf}"
