"""GPU: the fp32-in / fp32-accumulate modulated 3 x 3 convolution of csrc/nb_modconv.hip -- all 11 fp32-output kernels
(modconv3x3_up1_kernel <8,4,1,4,3>, <8,2,2,4,3>, <4,2,2,8,4>, <4,1,2,8,4>, <4,1,1,8,4>, the split-K <4,1,1,8,4,true>;
modconv3x3_up2_kernel <10,4>, <6,4>, <3,8>, <2,8>, <1,8>) and the five H2OUT twins of the up = 2 kernels -- each launched by
ctypes through nb_modconv3x3_f32 / nb_modconv3x3_up2_f32_h2 (NOT through ops.modulated_conv2d, whose routing sends large shapes
to the split-f16 kernels) and compared with a float64 evaluation of the layer with a LIVE epilogue: demodulation, per-sample /
shared / null noise, 1.5-sized bias, leaky ReLU, gain and a clamp that is reached; one case per kernel with the identity epilogue
of the training backward's dx launch.  No hook pins these kernels: the shape selects them, so every case first asks
nb_modconv3x3_variant and asserts the kernel the table names.  Case table, selector restatement, references:
tests/modconv_f32_refs.py, held without a GPU by tests/test_modconv_f32_refs_cpu.py.

Bound: 2e-6 of max|lin| x GAIN elementwise (conv_form_refs.B_FMT[0], what the hi / lo f16 kernels meet), through `within`; the
hand-off of the H2OUT twins: tol_handoff(0, ...) on ops.unpack_h2 of the output.  Outputs live in NaN-filled buffers with NaN
guards.  The packed weights lie inside a NaN-filled buffer as well, 128 floats of NaN behind them: the up = 1 kernels read up to
96 floats past the end of wpk when the last slice is ragged (docs/kernel_notes.md), into MFMA rows that are never stored -- a
stored output that depended on them would be NaN.

Every launch prints its observed error over the bound.  Worst error / bound observed on an MI355X per kernel, and the case:
    up1<8,4,1,4,3>        0.482  c_in 129 (192,136,8,8); short K: 0.179 (3,136,64,256), identity 0.153
    up1<8,2,2,4,3>        0.555  c_in 129 (384,40,8,8);  short K: 0.178 (12,36,64,256) identity
    up1<4,2,2,8,4>        0.545  c_in 129 (192,72,8,8);  c_in 35: 0.329 (3,72,64,256)
    up1<4,1,2,8,4>        0.484  c_in 129 (384,8,8,8);   c_in 35: 0.261 (3,36,64,256) identity
    up1<4,1,1,8,4>        0.488  c_in 129 (192,8,16,16); c_in 35: 0.254 (3,36,32,256) identity
    up1<4,1,1,8,4,true>   0.151  c_in 129 (1,72,8,64);   c_in 35: 0.088
    up2<10,4>             0.175  c_in 65 (12,8,64,256)      H2OUT twin 0.146
    up2<6,4>              0.188  c_in 65 (96,24,4,64)       H2OUT twin 0.147
    up2<3,8>              0.277  c_in 65 (64,40,32,8)       H2OUT twin 0.194
    up2<2,8>              0.181  c_in 65 (64,40,4,32)       H2OUT twin 0.130
    up2<1,8>              0.142  c_in 35 (3,72,8,8)         H2OUT twin 0.104
The up = 1 kernels other than split-K walk ONE fp32 accumulator per output through the whole K loop: their error grows with
sqrt(c_in) (1.1e-6 of max|lin| at c_in 129, 2.4e-6 .. 3.0e-6 at c_in 512 with the identity epilogue, where plain fp32 on the CPU
stays at 3e-7) -- figures and what follows from them in docs/kernel_notes.md."""
import ctypes
import functools

import pytest
import torch

import conv_form_refs as cf
import modconv_f32_refs as mr
from test_hip_conv_forms_f64 import _S, _check, report
from test_hip_step_kernels import GUARD, Out, P

pytestmark = pytest.mark.gpu

WPK_SLACK = 128                   # floats of NaN behind the packed weights


def _lib():
    from brushstroke_engine_amd import _lib
    return _lib.lib()


@functools.lru_cache(maxsize=None)
def _dev_inputs(up, n, ci, co, h, w):
    return {k: v.cuda() for k, v in cf.inputs(up, n, ci, co, h, w).items()}


@functools.lru_cache(maxsize=None)
def _guarded_wpk(up, n, ci, co, h, w):
    """(buffer, wpk): ops.pack_conv_weight's layout inside a NaN-filled buffer, GUARD floats before it and WPK_SLACK behind."""
    from brushstroke_engine_amd import ops
    wpk = ops.pack_conv_weight(_dev_inputs(up, n, ci, co, h, w)["w"], want_wsq=False)[0]
    assert list(wpk.shape) == [(ci + 7) // 8 * 8, 9, (co + 31) // 32 * 32]
    buf = torch.full([GUARD + wpk.numel() + WPK_SLACK], float("nan"), dtype=torch.float32, device=wpk.device)
    body = buf[GUARD:GUARD + wpk.numel()]
    body.copy_(wpk.flatten())
    assert body.data_ptr() % 16 == 0
    return buf, body


def _variant(lib, c):
    buf = ctypes.create_string_buffer(128)
    _check(lib.nb_modconv3x3_variant(c.n, c.h, c.w, c.co, c.up, buf, len(buf)), "variant")
    return buf.value.decode()


def _operands(c):
    """Device operands of a case: x split into x1 / x2 by slicing; the identity epilogue's zero bias and null noise."""
    up, n, ci, co, h, w = mr.shape_of(c)
    g = _dev_inputs(up, n, ci, co, h, w)
    x1 = g["x"][:, :c.c1].contiguous()
    x2 = g["x"][:, c.c1:].contiguous() if c.c2 else None
    bias = g["bias"] if c.epi == "live" else torch.zeros_like(g["bias"])
    hw_out = up * up * h * w
    nz = (P(g["noise"]), hw_out) if c.noise == "per" else (P(g["noise"][0]), 0) if c.noise == "shared" else (None, 0)
    keep = (x1, x2, bias) + _guarded_wpk(up, n, ci, co, h, w)
    return g, x1, x2, bias, nz, keep


@pytest.mark.parametrize("c", mr.CASES, ids=mr.case_id)
def test_f32_kernels_vs_float64(c):
    """nb_modconv3x3_f32 on every case of modconv_f32_refs.CASES: the library names the kernel the table names; the fp32 output
    within 2e-6 x max|lin| x GAIN of float64 elementwise, no output missing, guards untouched, NaN behind wpk without effect."""
    lib = _lib()
    up, n, ci, co, h, w = mr.shape_of(c)
    assert _variant(lib, c) == mr.kernel_name(c.variant)
    g, x1, x2, bias, nz, keep = _operands(c)
    r = mr.reference(c)
    y = Out([n, co, up * h, up * w], x1.device)
    what = "f32 " + mr.case_id(c)
    rc = lib.nb_modconv3x3_f32(P(x1), c.c1, P(x2), c.c2, P(keep[-1]), P(g["st"]), P(g["dco"]), *nz, P(bias), P(y.t), n, h, w, co, up,
                               *mr.epilogue_args(c), _S())
    _check(rc, what)
    torch.cuda.synchronize()
    worst = report(what, y.t, r["ref"], mr.B * r["scale"])
    print(f"[modconv-f32] {mr.kernel_name(c.variant)} {what}: err / bound {worst:.3f}, err / (max|lin| x gain of the launch) "
          f"{worst * mr.B * r['scale'] / (float(r['lin'].abs().max()) * mr.epilogue_args(c)[1]):.3e}")
    assert y.guards_untouched(), f"{what}: stray write"


def _h2_dest(c, dev):
    """The H2 destination of an up = 2 launch, [n, ceil(c_out / 8), 2, 2h, 2w, 8] f16: NaN where the kernel must write (whole groups
    of 4 channels up to ceil4(c_out)), zero in the half group behind them that it must not touch."""
    from brushstroke_engine_amd import ops
    out = Out(ops.h2_shape(c.n, c.co, 2 * c.h, 2 * c.w), dev, dtype=torch.float16)
    written = (c.co + 3) // 4 * 4
    if written % 8:
        out.t[:, -1, :, :, :, 4:] = 0
    return out, written


@pytest.mark.parametrize("c", [c for c in mr.CASES if mr.h2_allowed(c)], ids=mr.case_id)
def test_h2out_twins_vs_float64(c):
    """nb_modconv3x3_up2_f32_h2 (modconv3x3_up2_kernel<.., true>) on every up = 2 case, ragged c_out included: out_scale = the
    consumer's styles with row stride c_out; ops.unpack_h2 of the output within tol_handoff(0, ...) of float64 ref x next style;
    the channels between c_out and the next multiple of 4 written as zero, the half group behind them untouched, guards intact."""
    from brushstroke_engine_amd import ops
    lib = _lib()
    up, n, ci, co, h, w = mr.shape_of(c)
    assert _variant(lib, c) == mr.kernel_name(c.variant)
    g, x1, x2, bias, nz, keep = _operands(c)
    d, r = cf.inputs(up, n, ci, co, h, w), mr.reference(c)
    nst = g["nst"][:, :co].contiguous()                                                   # (row stride c_out)
    out, written = _h2_dest(c, x1.device)
    what = "h2 " + mr.case_id(c)
    alpha, gain, clamp = mr.epilogue_args(c)
    rc = lib.nb_modconv3x3_up2_f32_h2(P(x1), c.c1, P(x2), c.c2, P(keep[-1]), P(g["st"]), P(g["dco"]), *nz, P(bias), P(nst), P(out.t),
                                      n, h, w, co, alpha, gain, clamp, _S())
    _check(rc, what)
    torch.cuda.synchronize()
    want = cf.handoff_want(d, r["ref"], co)
    worst = report(what, ops.unpack_h2(out.t, co), want, cf.tol_handoff(0, r["scale"], d, want, co))
    print(f"[modconv-f32] {mr.kernel_name(c.variant)[:-1]}, true> {what}: err / bound {worst:.3f}")
    last = out.t[:, -1].float()                                                           # [n, hi / lo, H, W, 8]
    assert bool((last[..., co - (co - 1) // 8 * 8:] == 0).all()), f"{what}: channels past c_out are not zero"
    assert out.guards_untouched(), f"{what}: stray write"


def test_up2_refuses_more_input_channels_than_its_style_table():
    """c_in = 1025 > NB_STY_MAX at up = 2: NB_EINVAL with the launcher's message before any launch, y untouched, the stream usable."""
    from brushstroke_engine_amd import _lib as L
    lib = _lib()
    n, ci, co, h = 1, mr.STY_MAX + 1, 8, 4
    dev = torch.device("cuda")
    x = torch.zeros([n, ci, h, h], device=dev)
    wpk = torch.zeros([(ci + 7) // 8 * 8, 9, 32], device=dev)
    st, dco, bias = torch.ones([n, ci], device=dev), torch.ones([n, co], device=dev), torch.zeros([co], device=dev)
    y = Out([n, co, 2 * h, 2 * h], dev)
    rc = lib.nb_modconv3x3_f32(P(x), ci, None, 0, P(wpk), P(st), P(dco), None, 0, P(bias), P(y.t), n, h, h, co, 2, 1.0, 1.0, -1.0, _S())
    err = lib.nb_last_error().decode()
    assert rc == L.NB_EINVAL and f"modconv up2: c_in={ci} exceeds {mr.STY_MAX}" in err, (rc, err)
    torch.cuda.synchronize()
    assert bool(torch.isnan(y.buf).all()), "a refused launch wrote"
    assert float((torch.ones(8, device=dev) * 2).sum()) == 16.0
