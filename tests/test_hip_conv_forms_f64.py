"""GPU: every form of the split-f16 up=1 kernel (modconv3x3_up1_h3_kernel: 64- / 128-channel workgroups, 1 / 2 pixel rows per
wave, the round-3, software-pipelined and ping-pong K loops, H2 / f8 / f6 operands, persistent or not; modconv3x3_up1_h3s_kernel),
the older up=2 forms (modconv3x3_up2_h3_kernel: 12-, 8- and 5-row tiles, the 4-wave pair form, the 16-wide and 8-wide forms) and
the small-image kernels (nb_modconv3x3_up1_small_h3 / _up2_small_h3), each pinned with its debug hook and compared with a float64
evaluation of the layer through every output route -- fp32, hand-off in the form's own format, ToRGB from the accumulators,
ToRGB from the LDS image -- with a LIVE epilogue: demodulation, per-sample / shared / null noise, bias, leaky ReLU, gain and a
clamp that is reached.  References, bounds, case tables: tests/conv_form_refs.py (checked without a GPU by
tests/test_conv_form_refs_cpu.py: every workgroup's block of outputs lies on both sides of kink and clamp, and a wrong row order,
a clamp before the gain, a dropped channel group ... moves the reference by >= 20 bounds).

Outputs live in NaN-filled buffers with NaN guards (hand-off buffers: NaN where the producer writes, zero where it must not), and
every comparison goes through `within`, so a tile never written fails.  Every launch prints its observed error and bound.

Observed on an MI355X, worst error / bound over all forms, shapes and noise modes (all forms of one operand format agree to the
digits shown):
    up = 1   fp32       H2 0.26 (4.8e-6 of 1.8e-5)   f8 0.31 (9.0e-5 of 3.0e-4)   f6 0.18 (1.6e-4 of 8.9e-4)
             hand-off   H2 0.20 (5.9e-6 of 3.0e-5)   f8 0.23 (1.7e-4 of 7.6e-4); fp8(v / 4) plane 0.79 (0.250 of 0.315)
                        f6: hi slots and scale bytes equal the pack bit for bit, no field differs in any case
             ToRGB      logits H2 0.013, f8 0.027, f6 0.018; uvs / img / rgba <= 0.032; colors 0.27 (7.4e-8 of 2.8e-7)
    up = 2   fp32       H2 0.20 (2.2e-6 of 1.1e-5)   f8 0.38 (9.2e-5 of 2.4e-4)
             hand-off   H2 0.15 (2.8e-6 of 1.8e-5)   f8 0.24 (1.1e-4 of 4.8e-4); fp8(v / 4) plane 0.80 (0.250 of 0.313)
    small    |y - float64| / (max|lin| x GAIN): up = 1 <= 3.40e-7, up = 2 <= 6.06e-7  ->  SMALL_B = 4 x 6.06e-7 = 2.4e-6 (was: flat 5e-5)"""
import contextlib
import ctypes
import functools

import pytest
import torch

import conv_form_refs as cf
from test_hip_step_kernels import GUARD, Out, P, within
from test_hip_up2v_runs import _decode_f8

pytestmark = pytest.mark.gpu

# hook -> the value that restores the library's own choice
HOOKS = {"up1_rows": 0, "up1_v2": -1, "up1_pp": -1, "up1_persistent": -1, "up1_small": -1, "persistent_wgs_per_cu": 0,
         "up2_tile": 0, "up2_pair": -1, "up2_v2": -1, "up2v_rows": 0, "up2v_persistent": -1, "small_waves": 0, "small_blocks": 0}


def _lib():
    from brushstroke_engine_amd import _lib
    lib = _lib.lib()
    for h in HOOKS:
        f = getattr(lib, "nb_debug_set_" + h)
        f.argtypes, f.restype = [ctypes.c_int], None
    return lib


@contextlib.contextmanager
def pinned(lib, **hooks):
    """Set the named hooks; restore EVERY hook on the way out, whatever happened in between."""
    try:
        for h, v in hooks.items():
            getattr(lib, "nb_debug_set_" + h)(v)
        yield
    finally:
        for h, v in HOOKS.items():
            getattr(lib, "nb_debug_set_" + h)(v)


def _S():
    return torch.cuda.current_stream().cuda_stream


def _check(rc, what):
    from brushstroke_engine_amd import _lib
    _lib.check(rc, what)


def report(what, got, want, tol):
    """Print the observed error and the bound, then assert |got - want| <= tol elementwise with no value missing."""
    g, w_ = got.detach().double().cpu(), want.double().cpu()
    t = tol if torch.is_tensor(tol) else torch.tensor(float(tol), dtype=torch.float64)
    err = (g - w_).abs()
    fin = torch.isfinite(err)
    worst = float((err / t.expand_as(err))[fin].max()) if bool(fin.any()) else float("nan")
    print(f"[conv-forms] {what}: max err {float(err[fin].max()) if bool(fin.any()) else float('nan'):.3e}, bound {float(t.max()):.3e}, "
          f"worst err / bound {worst:.3f}")
    within(got, want, tol, what)
    return worst


def half_out(shape, dev, written):
    """A hand-off destination: `Out` of f16 whose first `written` channel groups are NaN (the producer must write them) and whose
    other groups are zero (it must not touch them)."""
    o = Out(shape, dev, dtype=torch.float16)
    o.t[:, written:] = 0
    return o


@functools.lru_cache(maxsize=None)
def _dev_inputs(up, n, ci, co, h, w):
    return {k: v.cuda() for k, v in cf.inputs(up, n, ci, co, h, w).items()}


@functools.lru_cache(maxsize=None)
def _packed(up, n, ci, co, h, w, fmt):
    """(activations in the operand format `fmt` with the styles folded in, packed weights)"""
    from brushstroke_engine_amd import ops
    g = _dev_inputs(up, n, ci, co, h, w)
    pack_x = (ops.pack_h2, ops.pack_h2f8, ops.pack_h2f6)[fmt]
    pack_w = (ops.pack_conv_weight_h3, ops.pack_conv_weight_h3f8, ops.pack_conv_weight_h3f6)[fmt]
    return pack_x(g["x"], g["st"]), pack_w(g["w"])


def _noise_args(g, noise, hw_out):
    """(pointer, sample stride) of a noise mode"""
    return (P(g["noise"]), hw_out) if noise == "per" else (P(g["noise"][0]), 0) if noise == "shared" else (None, 0)


def _check_f32(what, y, r, tol):
    worst = report(what + " fp32", y.t, r["ref"], tol)
    assert y.guards_untouched(), f"{what}: stray fp32 write"
    return worst


def _check_handoff(what, out, d, r, fmt, co, c_next, tol=None):
    """Decoded hand-off operand against float64 ref x next style; untouched channel groups stay zero; guards stay NaN.
    fmt = the container (0 H2, 1 f8); tol: the bound where the operands' format is not the container's (cf.tol_handoff_x)."""
    from brushstroke_engine_amd import ops
    want = cf.handoff_want(d, r["ref"], co)
    tol = cf.tol_handoff(fmt, r["scale"], d, want, co) if tol is None else tol
    body = out.t[:, :co // 8].contiguous()
    if fmt:
        v, v4 = _decode_f8(body, co)
        report(what + " hand-off fp8(v/4) plane", v4, want, cf.FP8_PLANE * float(want.abs().max()))
    else:
        v = ops.unpack_h2(body, co)
    report(what + " hand-off", v, want, tol)
    assert not out.t[:, co // 8:].contiguous().view(torch.int16).any(), f"{what}: channel groups past c_out written"
    assert out.guards_untouched(), f"{what}: stray hand-off write"


def _check_f6_handoff(what, out, y, g, co):
    """The f6 hand-off has no host decoder in formats.py: the pack-equality of test_f6_handoff_equals_pack on these live-epilogue
    inputs -- the producer's f6 output == its own fp32 output (held to float64 by the fp32 route) packed with the consumer's styles:
    hi slots and scale bytes bit for bit, fields equal except on rounding ties of the 6-bit grid."""
    from brushstroke_engine_amd import ops
    assert not torch.isnan(y.t).any(), f"{what}: fp32 outputs never written"
    ref = ops.pack_h2f6(y.t.contiguous(), g["nst"][:, :co].contiguous())
    got = out.t[:, :co // 8].contiguous()
    assert torch.equal(got[:, :, 0].contiguous().view(torch.int16), ref[:, :, 0].contiguous().view(torch.int16)), f"{what}: hi slots differ"
    g_hi, g_xl, g_x, g_sc = ops.unpack_h2f6(got, co)
    r_hi, r_xl, r_x, r_sc = ops.unpack_h2f6(ref, co)
    assert torch.equal(g_sc, r_sc), f"{what}: scale bytes differ"
    fx, fl = float((g_x != r_x).float().mean()), float((g_xl != r_xl).float().mean())
    ex = float((g_x - r_x).abs().max())
    print(f"[conv-forms] {what} f6 hand-off vs pack: fields differing {fx:.2e} (x) {fl:.2e} (xl), bound 1e-3; max |x - x_pack| {ex:.3e}, "
          f"bound {0.07 * float(r_x.abs().max()):.3e}")
    assert fx < 1e-3 and fl < 1e-3, (what, fx, fl)
    assert ex <= 0.07 * float(r_x.abs().max()), (what, ex)
    assert not out.t[:, co // 8:].contiguous().view(torch.int16).any(), f"{what}: channel groups past c_out written"
    assert out.guards_untouched(), f"{what}: stray hand-off write"


def _torgb_outputs(n, hw, dev):
    o = {"logits": Out([n, 3, hw], dev), "uvs": Out([n, 3, hw], dev), "img": Out([n, 3, hw], dev), "colors_out": Out([n, 9], dev),
         "rgba_f32": Out([n, 4, hw], dev)}
    u8 = torch.full([n * hw * 4 + 2 * GUARD], 0xA5, dtype=torch.uint8, device=dev)
    return o, u8


def _torgb_args(g, o, u8, shape, co):
    from brushstroke_engine_amd import _lib
    mode, clamp, ucol, sfk = cf.TORGB_SETTINGS[shape]
    t = _lib.NbTorgbArgs()
    t.styles, t.w, t.bias, t.color_bias = P(g["tst"]), P(g["tw"]), P(g["tb"]), P(g["cb"])
    t.logits, t.uvs, t.img, t.colors_out = P(o["logits"].t), P(o["uvs"].t), P(o["img"].t), P(o["colors_out"].t)
    t.user_colors, t.sfactor = (P(g["uc"]) if ucol else None), (P(g["sf"]) if sfk else None)
    t.rgba_f32, t.rgba_u8 = P(o["rgba_f32"].t), u8.data_ptr() + GUARD
    t.styles_stride_n, t.render_mode, t.clamp = co + 12, mode, clamp
    return t


def _check_torgb(what, o, u8, d, r, fmt, co, shape, n, hw):
    ref, amb = cf.torgb_reference(d, r["ref"], co, shape, cf.tol_f32(fmt, r["scale"]))
    assert float(amb.double().mean()) < 0.1, "too many pixels at the f = 0 threshold"
    for k in ("logits", "uvs", "img", "colors_out", "rgba_f32"):
        got = o[k].t
        want, tol = ref[k]
        if k == "rgba_f32":
            keep = ~amb.unsqueeze(1).expand_as(want)
            got, want, tol = got.cpu()[keep], want[keep], tol.expand_as(want)[keep]
        report(f"{what} torgb {k}", got, want, tol)
        assert o[k].guards_untouched(), f"{what} {k}: stray write"
    body = u8[GUARD:GUARD + n * hw * 4].view(n, hw, 4)
    assert bool((u8[:GUARD] == 0xA5).all() and (u8[GUARD + n * hw * 4:] == 0xA5).all()), f"{what}: stray rgba_u8 write"
    mine = (o["rgba_f32"].t * 255).clamp(0, 255).to(torch.uint8).permute(0, 2, 1)
    assert torch.equal(body, mine), f"{what}: rgba_u8 != trunc(clamp(rgba_f32 * 255))"


# ---------------------------------------------------------------------------------------------------------------------
# up = 1
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form,shape,route", cf.up1_cases(), ids=lambda v: str(v))
def test_up1_forms_vs_float64(form, shape, route):
    """nb_modconv3x3_up1_h3_ex with the form pinned (nb_debug_set_up1_rows / _up1_v2 / _up1_pp / _up1_persistent / _up1_small;
    shape P with nb_debug_set_persistent_wgs_per_cu(1): 280 items on 256 workgroups) against float64: fp32 within B x max|lin| x GAIN
    (B = 2e-6 H2, 4e-5 f8, 8e-5 f6), hand-off as in test_up2v_runs_vs_float64 (c_next > c_out, next_stride > c_next; f6: pack-equality),
    fused ToRGB within _torgb_ref's bounds with the conv bound carried into the logits (render mode 1, ToRGB clamp 0.5, partly-NaN
    user colors and an sfactor each occur: conv_form_refs.TORGB_SETTINGS).  Routes `f32-shared` / `f32-null`: shared noise
    (stride 0) and null noise with a live bias.  Shape C (odd number of channel groups) runs the round-3 loop whatever is asked."""
    from brushstroke_engine_amd import ops
    lib = _lib()
    f = cf.UP1_FORMS[form]
    fmt = f["fmt"]
    n, ci, co, h, w = UP = cf.UP1_SHAPES[shape]
    noise = {"f32-shared": "shared", "f32-null": "null"}.get(route, "per")
    d, g = cf.inputs(1, *UP), _dev_inputs(1, *UP)
    r = cf.reference(1, *UP, noise)
    xh, wp = _packed(1, *UP, fmt)
    dev = xh.device
    common = (P(g["dco"]),) + _noise_args(g, noise, h * w) + (P(g["bias"]),)
    tail = (n, h, w, co, cf.ALPHA, cf.GAIN, cf.CLAMP, _S())
    what = f"up1 {form} {shape} {route}"
    c_next = cf.c_next_of(co)
    y = out = o = u8 = None
    with pinned(lib, up1_rows=f["rows"], up1_v2=f["v2"], up1_pp=f["pp"], up1_persistent=f["persist"], up1_small=f["small"],
                persistent_wgs_per_cu=1 if shape == "P" else 0):
        if route.startswith("f32") or route == "torgb-tap" or (route == "handoff" and fmt == 2):
            y = Out([n, co, h, w], dev)
        if route.startswith("f32") or (route == "handoff" and fmt == 2):
            _check(lib.nb_modconv3x3_up1_h3_ex(P(xh), ci, P(wp), *common, P(y.t), None, None, 0, 0, None, fmt, 0, *tail), what)
        if route == "handoff":
            out = half_out(ops.h2_shape(n, c_next, h, w), dev, co // 8)
            _check(lib.nb_modconv3x3_up1_h3_ex(P(xh), ci, P(wp), *common, None, P(out.t), P(g["nst"]), c_next + 8, c_next, None, fmt, fmt,
                                               *tail), what)
        if route.startswith("torgb"):
            o, u8 = _torgb_outputs(n, h * w, dev)
            t = _torgb_args(g, o, u8, shape, co)
            _check(lib.nb_modconv3x3_up1_h3_ex(P(xh), ci, P(wp), *common, None if y is None else P(y.t), None, None, 0, 0, ctypes.byref(t),
                                               fmt, 0, *tail), what)
        torch.cuda.synchronize()
    if route.startswith("f32") or route == "torgb-tap":
        _check_f32(what, y, r, cf.tol_f32(fmt, r["scale"]))
    if route == "handoff":
        if fmt == 2:
            _check_f6_handoff(what, out, y, g, co)
        else:
            _check_handoff(what, out, d, r, fmt, co, c_next)
    if route.startswith("torgb"):
        _check_torgb(what, o, u8, d, r, fmt, co, shape, n, h * w)


# ---------------------------------------------------------------------------------------------------------------------
# the older up = 2 forms
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form,fmt,ci,co,h,w,n,route", cf.up2_cases(), ids=lambda v: str(v))
def test_up2_older_forms_vs_float64(form, fmt, ci, co, h, w, n, route):
    """nb_modconv3x3_up2_h3_ex with nb_debug_set_up2_v2(0) and the tile pinned (nb_debug_set_up2_tile 12 / 8 / 5, nb_debug_set_up2_pair)
    on the five shapes of test_up2v_runs_vs_float64; the 16-wide form on 8 x 16, 12 x 16 (ragged) and 24 x 16 (three tile rows),
    the 8-wide form on 8 x 8 and 16 x 8.  16 x 8 (w == 8 with h > 8) is accepted by the launcher and was run by nothing; read before
    it was launched: modconv3x3_up2_h3_kernel<.., 8, 8, ..> takes tiles_y = ceil(h / 8) tile rows from the launcher, guards every
    halo load by 0 <= gy < H and 0 <= gx < W (else the zero page), every noise read by oy < 2 H (ox < 2 TQW = 2 W), every store by
    qi < H with qj < TQW = W, and indexes its LDS planes by the tile-local position only -- the code of the 16-wide instantiation
    that the 16 x 16 layer has always run on two tile rows; in bounds.  fp32 and hand-off (H2 -> H2, f8 -> f8), bounds as above."""
    from brushstroke_engine_amd import ops
    lib = _lib()
    UP = (n, ci, co, h, w)
    d, g = cf.inputs(2, *UP), _dev_inputs(2, *UP)
    r = cf.reference(2, *UP)
    xh, wp = _packed(2, *UP, fmt)
    dev = xh.device
    tile, pair = cf.UP2_FORMS[form][:2] if form in cf.UP2_FORMS else (0, 0)
    common = (P(g["dco"]), P(g["noise"]), 4 * h * w, P(g["bias"]))
    tail = (n, h, w, co, cf.ALPHA, cf.GAIN, cf.CLAMP, _S())
    what = f"up2 {form} {cf.FMT_NAME[fmt]} {ci}->{co} {h}x{w} n{n} {route}"
    c_next = cf.c_next_of(co)
    with pinned(lib, up2_v2=0, up2_tile=tile, up2_pair=pair):
        if route == "f32":
            y = Out([n, co, 2 * h, 2 * w], dev)
            _check(lib.nb_modconv3x3_up2_h3_ex(P(xh), ci, P(wp), *common, P(y.t), None, None, 0, 0, fmt, 0, *tail), what)
        else:
            out = half_out(ops.h2_shape(n, c_next, 2 * h, 2 * w), dev, co // 8)
            _check(lib.nb_modconv3x3_up2_h3_ex(P(xh), ci, P(wp), *common, None, P(out.t), P(g["nst"]), c_next + 8, c_next, fmt, fmt, *tail),
                   what)
        torch.cuda.synchronize()
    if route == "f32":
        _check_f32(what, y, r, cf.tol_f32(fmt, r["scale"]))
    else:
        _check_handoff(what, out, d, r, fmt, co, c_next)


# ---------------------------------------------------------------------------------------------------------------------
# the small-image kernels
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("up,n,c1,c2,co,h,waves,blocks,noise", cf.small_cases(), ids=lambda v: str(v))
def test_small_kernels_vs_float64(up, n, c1, c2, co, h, waves, blocks, noise):
    """nb_modconv3x3_up1_small_h3 / nb_modconv3x3_up2_small_h3 (fp32 input, styles folded in by the kernel; up = 2: four phase
    kernels with the FIR folded into the weights in fp32) with the same live epilogue and the clamp reached: 4 x 4 images at n = 3
    (two samples per tile, half-empty last tile), 8 x 8, 16 x 16, 64 x 64 (the w >= 32 path); 4 / 8 K-splitting waves; two-block tiles
    where the launcher's can_two holds; the concatenated second input (up = 2); per-sample, shared and null noise.
    Bound: |y - float64| <= SMALL_B x max|lin| x GAIN (conv_form_refs.SMALL_B = 4 x the worst ratio observed over these cases, at most
    the flat 5e-5 these kernels had).  Measured on an MI355X, ratio |y - float64| / (max|lin| x GAIN), the same for 4 and 8 waves and
    for one and two blocks per tile (per-sample / shared / null noise):
        up = 1   4 x 4: 2.78e-7 / 2.73e-7 / 3.40e-7    8 x 8: 3.12e-7 / 3.12e-7 / 3.05e-7
                 16 x 16: 2.83e-7 / 2.83e-7 / 2.89e-7  64 x 64: 3.06e-7 / 2.91e-7 / 2.88e-7
        up = 2   4 x 4: 4.15e-7 (with the second input 4.64e-7) / 4.46e-7 / 4.16e-7    8 x 8: 4.99e-7 (6.06e-7) / 4.99e-7 / 5.61e-7
                 16 x 16: 5.01e-7 (4.81e-7) / 5.01e-7 / 5.06e-7                          64 x 64: 4.80e-7 (6.02e-7) / 4.80e-7 / 4.90e-7
    worst 6.06e-7 -> SMALL_B = 2.424e-6, a twentieth of the flat 5e-5."""
    from brushstroke_engine_amd import ops
    from oracle import neube_oracle as orc
    lib = _lib()
    ci = c1 + c2
    UP = (n, ci, co, h, h)
    g = _dev_inputs(up, *UP)
    r = cf.reference(up, *UP, noise)
    dev = g["x"].device
    wp = ops.pack_conv_weight_h3(g["w"]) if up == 1 else ops.pack_conv_weight_h3_up2_phases(g["w"], orc.setup_filter().to(dev))
    x1 = g["x"][:, :c1].contiguous()
    x2 = g["x"][:, c1:].contiguous() if c2 else None
    y = Out([n, co, up * h, up * h], dev)
    nz = _noise_args(g, noise, up * up * h * h)
    tail = (P(g["bias"]), P(y.t), n, h, h, co, cf.ALPHA, cf.GAIN, cf.CLAMP, _S())
    what = f"small up{up} n{n} {c1}+{c2}->{co} {h}x{h} waves{waves} blocks{blocks} noise-{noise}"
    with pinned(lib, small_waves=waves, small_blocks=blocks):
        if up == 1:
            rc = lib.nb_modconv3x3_up1_small_h3(P(x1), c1, P(wp), P(g["st"]), P(g["dco"]), *nz, *tail)
        else:
            rc = lib.nb_modconv3x3_up2_small_h3(P(x1), c1, P(x2), c2, P(wp), P(g["st"]), P(g["dco"]), *nz, *tail)
        _check(rc, what)
        torch.cuda.synchronize()
    worst = _check_f32(what, y, r, cf.SMALL_FLAT * r["scale"])
    print(f"[conv-forms] {what}: err / (max|lin| x GAIN) = {worst * cf.SMALL_FLAT:.3e}")
    within(y.t, r["ref"], cf.SMALL_B * r["scale"], what + " (SMALL_B)")
