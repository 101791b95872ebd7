"""GPU: the geometry encoder's kernels (csrc/nb_encoder.hip) against float64 on every output route.

    enc_conv3x3_h3_kernel        all 16 <STRIDE, LW, OUT, F8> instantiations; fp32, plain H2 / f8 containers, and the hand-off into channel
                                 groups cg0 .. of a wider consumer tensor, with and without the consumer's styles (oscale, both signs,
                                 oscale_stride > c_out) -- through the 32-wide tiles' epilogue (straight from the accumulators) and the
                                 16-wide tiles' (staged through LDS); nb_enc_conv3x3_ex and nb_enc_conv3x3_h3_handoff itself
    enc_conv3x3_small_h3_kernel  the 32-position split-K tiles: masked tile rows, ragged 32-channel slices, idle K-split waves
    enc_stem7x7_kernel           three preprocessings x H2 / f8 output, a single tile and 2 x 2 tiles
    enc_upsample2x_h2_kernel     H2 / f8 output, 2 x 2 and odd non-square inputs, and a launch past the 16384-workgroup grid cap

References, decoders, bounds and case tables: tests/enc_refs.py (checked without a GPU by tests/test_enc_refs_cpu.py: every workgroup's
block of outputs has pre-activations of both signs, and replicate padding, a stride-2 window from 2i, the scale before the LeakyReLU, a
wrong scale-row stride, a wrong slice's bias, a dropped chunk ... move the reference by >= 20 bounds).

Every destination lies in a guarded buffer of NaNs (f16 containers: the bit pattern 0x7E00): a value never written fails, and the
guards and every word outside the (cg0, c_out) window must keep their bits.  Every launch prints its observed error and bound.

Observed on an MI355X, worst error / bound of each family (115 cases, 1.6 - 1.9 s); all bounds are the project's own, none was measured:
    large tiles   fp32          H2 operands 2.7e-6 of 8.3e-6 (0.33)   f8 operands 5.3e-5 of 1.7e-4 (0.32)
                  H2 container  H2 3.4e-6 of 1.0e-5 (0.34), x styles 4.2e-6 of 1.6e-5 (0.26)   f8 6.2e-5 of 2.0e-4 (0.31), x styles 0.27
                  f8 container  H2 6.0e-5 of 1.1e-4 (0.56), x styles 1.2e-4 of 1.8e-4 (0.68)   f8 8.7e-5 of 2.9e-4 (0.30), x styles 0.24
                  fp8(v / 4)    0.71 of the bound at worst (0.43 of 0.60)
                  err / (max|lin| x max(1, max|oscale|)): H2 operands 2.7e-7 ... 8.7e-7 (fp32, H2 container), f8 operands 9.6e-6 ... 1.3e-5 (fp32)
    split-K tiles fp32 3.3e-6 of 7.3e-6 (0.46), H2 container 3.2e-6 of 1.0e-5 (0.31); err / max|lin| 2.6e-7 ... 9.1e-7 (c_in 256 at the top)
    stem          H2 container 9.0e-7 of 8.0e-6 (0.11), err / max|lin| 2.1e-7 ... 2.9e-7 over the six (size, preprocessing) cases: inside
                  B_FMT[0] = 2e-6, so STEM_B is that and no measured constant; f8 container 6.1e-5 of 1.2e-4 (0.52), plane 0.66
    bilinear      H2 container 5.2e-7 of 3.0e-6 (0.17); f8 container 5.7e-5 of 8.4e-5 (0.68), plane 0.55; past the grid cap 3.1e-5 of 8.1e-5"""
import functools

import numpy as np
import pytest
import torch

import enc_refs as er

pytestmark = pytest.mark.gpu

GUARD = 64                                            # elements before and after every destination (keeps 16-byte alignment)
NAN_BITS = {torch.float16: 0x7E00, torch.float32: 0x7FC00000}
INT_OF = {torch.float16: torch.int16, torch.float32: torch.int32}


class Dest:
    """A destination tensor of `shape` inside a NaN-filled buffer with GUARD elements on either side; `bits` = the buffer as integers."""

    def __init__(self, shape, dtype):
        numel = int(np.prod(shape))
        self.buf = torch.full([numel + 2 * GUARD], float("nan"), dtype=dtype, device="cuda")
        self.t = self.buf[GUARD:GUARD + numel].view(shape)
        self.nan = NAN_BITS[dtype]
        self.bits = self.buf.view(INT_OF[dtype])
        assert bool((self.bits == self.nan).all())

    def guards_untouched(self):
        return bool((self.bits[:GUARD] == self.nan).all() and (self.bits[-GUARD:] == self.nan).all())

    def untouched(self, mask=None):
        """The guards and the words of t under `mask` (None: all of t) still hold the fill pattern, bit for bit."""
        body = self.t.view(self.bits.dtype)
        inside = (body == self.nan) if mask is None else (body[mask.to(body.device)] == self.nan)
        return self.guards_untouched() and bool(inside.all())


def _lib():
    from brushstroke_engine_amd import _lib
    return _lib.lib()


def _check(rc, what):
    from brushstroke_engine_amd import _lib
    _lib.check(rc, what)


def _S():
    return torch.cuda.current_stream().cuda_stream


def P(t):
    return None if t is None else t.data_ptr()


def report(what, got, want, tol, scale=None):
    """Print the observed error, the bound and (scale given) the error relative to it; then assert |got - want| <= tol with no value
    missing.  Returns the worst error."""
    g, w_ = got.detach().double().cpu(), want.double().cpu()
    assert g.shape == w_.shape, (what, g.shape, w_.shape)
    missing = int(torch.isnan(g).sum())
    err = (g - w_).abs()
    worst = float(err[~torch.isnan(err)].max()) if missing < err.numel() else float("nan")
    rel = "" if scale is None else f", err / scale {worst / scale:.3e}"
    print(f"[enc-routes] {what}: max err {worst:.3e}, bound {tol:.3e}, err / bound {worst / tol:.3f}{rel}")
    assert missing == 0, f"{what}: {missing} outputs never written"
    assert worst <= tol, f"{what}: {int((err > tol).sum())} of {err.numel()} outside the bound (worst {worst / tol:.3g}x)"
    return worst


@pytest.fixture(scope="module", autouse=True)
def _release_device_operands():
    """The cached device operands live as long as this module's tests, not for the rest of the suite."""
    yield
    _dev_conv.cache_clear()


@functools.lru_cache(maxsize=None)
def _dev_conv(kind, stride, ci, co, ho, wo, in_fmt):
    """Device operands of a conv shape: activations in the operand format, packed weights, bias, the scale buffer."""
    from brushstroke_engine_amd import encoder as encmod, ops
    d = er.conv_inputs(kind, stride, ci, co, ho, wo)
    x = d["x"].cuda()
    if in_fmt:
        xp = ops.pack_h2f8(x, torch.ones(x.shape[0], ci, device="cuda"))
        wp = torch.from_numpy(encmod.pack_enc_weight_f8(d["w"].numpy())).cuda()
    else:
        xp = ops.pack_h2(x)
        wp = torch.from_numpy(encmod.pack_enc_weight_h3(d["w"].numpy())).cuda()
    return dict(x=xp, w=wp, b=d["b"].cuda(), osc=d["osc_buf"].cuda())


def _check_container(what, dest, out_fmt, cg0, co, want, tol, scale):
    t = dest.t.cpu()
    if out_fmt:
        v, plane, mask = er.decode_f8(t, cg0, co)
        report(what + " fp8(v/4) plane", plane, want, er.tol_plane(want))
    else:
        v, mask = er.decode_h2(t, cg0, co)
    worst = report(what, v, want, tol, scale)
    assert dest.untouched(mask), f"{what}: a word outside channel groups {cg0} .. {cg0 + co // 8 - 1}, or a guard, was written"
    return worst


def _run_conv(kind, small, stride, in_fmt, ci, co, ho, wo, route, api, what):
    lib = _lib()
    g = _dev_conv(kind, stride, ci, co, ho, wo, in_fmt)
    d = er.conv_inputs(kind, stride, ci, co, ho, wo)
    lin, want, osc = er.conv_want(kind, stride, ci, co, ho, wo, route)
    out_fmt, win, scaled = er.ROUTES[route]
    n, h_in, w_in = er.N_CONV, stride * ho, stride * wo
    cg0 = er.WIN_CG0 if win else 0
    c8_total = cg0 + co // 8 + er.WIN_EXTRA if win else (co // 8 if out_fmt else 0)
    osc_ptr = g["osc"].data_ptr() + 4 * er.OSC_OFF if scaled else None
    ostride = d["ostride"] if scaled else 0
    if out_fmt is None:
        dest = Dest([n, co, ho, wo], torch.float32)
    else:
        dest = Dest([n, max(c8_total, co // 8), 2, ho, wo, 8], torch.float16)
    lib.nb_debug_set_enc_small(small)
    try:
        if api == "handoff":
            rc = lib.nb_enc_conv3x3_h3_handoff(P(g["x"]), ci, P(g["w"]), P(g["b"]), P(dest.t), osc_ptr, ostride, c8_total, cg0, out_fmt,
                                               n, h_in, w_in, co, stride, er.SLOPE, _S())
        else:
            y32, yh2 = (P(dest.t), None) if out_fmt is None else (None, P(dest.t))
            rc = lib.nb_enc_conv3x3_ex(P(g["x"]), ci, P(g["w"]), P(g["b"]), y32, yh2, osc_ptr, ostride, c8_total, cg0, in_fmt, out_fmt or 0,
                                       n, h_in, w_in, co, stride, er.SLOPE, _S())
        _check(rc, what)
        torch.cuda.synchronize()
    finally:
        lib.nb_debug_set_enc_small(-1)
    tol = er.tol_route(in_fmt, route, lin, want, osc)
    scale = float(lin.abs().max()) * (1.0 if osc is None else max(1.0, float(osc.abs().max())))
    if out_fmt is None:
        worst = report(what, dest.t, want, tol, scale)
        assert dest.guards_untouched(), f"{what}: stray fp32 write"
        return worst
    return _check_container(what, dest, out_fmt, cg0, co, want, tol, scale)


@pytest.mark.parametrize("stride,tile,in_fmt,ci,co,ho,wo,route,api", er.large_cases(), ids=lambda v: str(v))
def test_large_tiles_vs_float64(stride, tile, in_fmt, ci, co, ho, wo, route, api):
    """enc_conv3x3_h3_kernel (nb_debug_set_enc_small(0)) through nb_enc_conv3x3_ex / nb_enc_conv3x3_h3_handoff, n = 3: fp32 within
    B_FMT[in_fmt] x max|lin| x max(1, max|oscale|) (2e-6 H2 operands, 4e-5 f8), decoded containers within that + KEEP_FMT[out_fmt] x
    max|want| (2^-21 H2, 2e-5 f8), the fp8(v / 4) plane within 0.07 max|want|; every word outside the window and the guards untouched."""
    what = f"large s{stride} {tile} in-{('h2', 'f8')[in_fmt]} {ci}->{co} {ho}x{wo} {route} {api}"
    _run_conv(0, 0, stride, in_fmt, ci, co, ho, wo, route, api, what)


@pytest.mark.parametrize("stride,ci,co,ho,wo,route", er.SMALL, ids=lambda v: str(v))
def test_small_tiles_vs_float64(stride, ci, co, ho, wo, route):
    """enc_conv3x3_small_h3_kernel (nb_debug_set_enc_small(1); H2 operands), n = 3, same bounds: 4 x 4 outputs (half of the 8-row tile
    masked) from both strides, 6 x 8 (a masked half tile behind a full one), 8 x 8, 16 x 16, the 32-wide one-row tile; c_in 16 (three idle
    K-split waves), 48, 256; c_out 8, 40 (ragged 32-slice), 64."""
    what = f"small s{stride} {ci}->{co} {ho}x{wo} {route}"
    _run_conv(1, 1, stride, 0, ci, co, ho, wo, route, "ex", what)


@pytest.mark.parametrize("n,h,w,pre,out_fmt", er.STEM, ids=lambda v: str(v))
def test_stem_vs_float64(n, h, w, pre, out_fmt):
    """nb_enc_stem7x7_f32_h2_ex: decoded output within STEM_B x max|lin| + KEEP_FMT[out_fmt] x max|want|; f8: the fp8(v / 4) plane."""
    lib = _lib()
    d = er.stem_inputs(n, h, w)
    lin, want = er.stem_ref(d["x"], d["w"], d["b"], pre)
    w50 = torch.zeros(64, 50)
    w50[:, :49] = d["w"].reshape(64, 49)
    xd, wd, bd = d["x"].cuda(), w50.cuda(), d["b"].cuda()
    dest = Dest([n, 8, 2, h, w, 8], torch.float16)
    what = f"stem {h}x{w} preproc {pre} out-{('h2', 'f8')[out_fmt]}"
    _check(lib.nb_enc_stem7x7_f32_h2_ex(P(xd), P(wd), P(bd), P(dest.t), out_fmt, n, h, w, pre, er.SLOPE, _S()), what)
    torch.cuda.synchronize()
    _check_container(what, dest, out_fmt, 0, 64, want, er.tol_decoded(0, out_fmt, lin, want, rel=er.STEM_B), float(lin.abs().max()))


@pytest.mark.parametrize("n,c,h,w,out_fmt,sampled", er.UPSAMPLE, ids=lambda v: str(v))
def test_upsample_vs_float64(n, c, h, w, out_fmt, sampled):
    """nb_enc_upsample2x_h2_ex: decoded output within UP_B x max|x| + KEEP_FMT[out_fmt] x max|want| of the float64 blend at the shared fp32
    coordinates.  The case past the grid cap (6.3 M items on 16384 x 256 threads) is compared at 65 551 sampled positions; that every
    slot of it was written is checked on the device."""
    lib = _lib()
    x = er.upsample_input(n, c, h, w)
    xd = x.cuda()
    dest = Dest([n, c // 8, 2, 2 * h, 2 * w, 8], torch.float16)
    what = f"upsample {n}x{c}x{h}x{w} out-{('h2', 'f8')[out_fmt]}"
    _check(lib.nb_enc_upsample2x_h2_ex(P(xd), P(dest.t), out_fmt, n, c, h, w, _S()), what)
    torch.cuda.synchronize()
    if not sampled:
        want = er.upsample_ref(x)
        _check_container(what, dest, out_fmt, 0, c, want, er.tol_upsample(x, out_fmt, want), float(x.abs().max()))
        return
    assert dest.guards_untouched(), f"{what}: stray write"
    assert not bool((dest.t.view(torch.int16) == dest.nan).any()), f"{what}: slots never written"
    ns, oys, oxs = er.upsample_sample_points(n, h, w)
    want = er.upsample_ref_at(x, ns, oys, oxs)                                      # [K, c]
    picked = dest.t[ns.cuda(), :, :, oys.cuda(), oxs.cuda()].cpu()                  # [K, c8, 2, 8]
    v, plane, _ = er.decode_f8(picked[:, :, :, None, None, :], 0, c)
    want = want[:, :, None, None]
    report(what + " fp8(v/4) plane", plane, want, er.tol_plane(want))
    report(what, v, want, er.tol_upsample(x, out_fmt, want), float(x.abs().max()))


NB_OK, NB_EINVAL = 0, -1                              # include/neube_hip.h


@pytest.mark.parametrize("why,api,kw", [
    ("the base arguments, accepted", "handoff", dict()),
    ("the base arguments through nb_enc_conv3x3_ex, accepted", "ex", dict()),
    ("f8 hand-off with odd cg0", "handoff", dict(out_fmt=1, cg0=1, c8_total=12)),
    ("f8 hand-off with c_out % 16 != 0", "handoff", dict(out_fmt=1, co=24, c8_total=12)),
    ("c8_total < cg0 + c_out / 8", "ex", dict(cg0=2, c8_total=7)),
    ("oscale_stride < c_out", "handoff", dict(scaled=True, ostride=47, c8_total=12)),
    ("hand-off on a shape only the small tiles take", "handoff", dict(ho=8, wo=8, c8_total=12)),
], ids=["accepted-handoff", "accepted-ex", "odd-cg0-f8", "c_out-24-f8", "c8_total-short", "oscale_stride-short", "small-tiles-only"])
def test_launcher_rejects_bad_handoff_arguments(why, api, kw):
    """The launcher's argument checks: NB_EINVAL, nothing launched, the destination untouched.  Every rejected case differs from the
    base arguments in the named argument alone; the base arguments themselves are accepted through both entry points (NB_OK, every
    word of the window written -- zeros, from zero operands --, the rest untouched), so no case is rejected for another reason."""
    lib = _lib()
    a = dict(out_fmt=0, cg0=2, c8_total=12, co=48, scaled=False, ostride=72, ho=16, wo=16)
    a.update(kw)
    ci, co, ho, wo = 16, a["co"], a["ho"], a["wo"]
    x = torch.zeros([er.N_CONV, 2, 2, ho, wo, 8], dtype=torch.float16, device="cuda")
    wp = torch.zeros([1, 3, 3, 2, 2, 128, 8], dtype=torch.float16, device="cuda")
    b = torch.zeros(co, device="cuda")
    osc = torch.ones(er.N_CONV * 72 + 8, device="cuda")
    dest = Dest([er.N_CONV, 12, 2, ho, wo, 8], torch.float16)
    osc_ptr = P(osc) if a["scaled"] else None
    if api == "handoff":
        rc = lib.nb_enc_conv3x3_h3_handoff(P(x), ci, P(wp), P(b), P(dest.t), osc_ptr, a["ostride"], a["c8_total"], a["cg0"], a["out_fmt"],
                                           er.N_CONV, ho, wo, co, 1, er.SLOPE, _S())
    else:
        rc = lib.nb_enc_conv3x3_ex(P(x), ci, P(wp), P(b), None, P(dest.t), osc_ptr, a["ostride"], a["c8_total"], a["cg0"], 0, a["out_fmt"],
                                   er.N_CONV, ho, wo, co, 1, er.SLOPE, _S())
    torch.cuda.synchronize()
    if not kw:
        assert rc == NB_OK, f"{why}: rc {rc}"
        mask = er.outside_mask(dest.t, a["cg0"], co)
        assert dest.untouched(mask), f"{why}: a word outside the window was written"
        assert not bool((dest.t.view(torch.int16)[~mask.cuda()] == dest.nan).any()), f"{why}: words of the window never written"
        return
    assert rc == NB_EINVAL, f"{why}: rc {rc}, expected NB_EINVAL"
    assert dest.untouched(), f"{why}: the destination was written"
