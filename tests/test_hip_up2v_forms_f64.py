"""GPU: all 36 instantiations of the pipelined up=2 kernel (modconv3x3_up2v_kernel, csrc/nb_modconv_up2v.hip: operand format H2 / f8 /
f6 / f8 hi-only x output fp32 / H2 container / f8 container x 12-row persistent / 12-row one workgroup per tile / 13-row tiles),
each pinned with its hooks (nb_debug_set_up2_v2(1), nb_debug_set_up2v_rows, nb_debug_set_up2v_persistent) and compared with a
float64 evaluation of the layer with a LIVE epilogue -- demodulation, per-sample / shared / null noise, bias, leaky ReLU, gain, a
clamp that every workgroup reaches -- at K loops of 1, 4, 5 and 7 chunks, ragged c_out (36, 48, 96), one to four tile columns and
every cross-format hand-off (H2 -> f8, f8 -> H2, f6 -> either, hi-only -> either; c_next > c_out, next_stride > c_next).  Beyond the
forms: the persistent tile loop (280 / 282 items on 256 workgroups: second iterations in the XCD-renumbered and in the plain item
order), the in-kernel noise (NbNoiseSrc) at every form, and the launcher's own selection (up2v or not, 12 or 13 rows, four
persistent workgroups per CU) with every hook at its default.  References, bounds, case tables: tests/conv_form_refs.py, checked
without a GPU by tests/test_conv_form_refs_cpu.py (every workgroup's block on both sides of kink and clamp; a second item rendered
with its first item's channel tables or noise tile moves the reference by >= 20 bounds).

Bounds (conv_form_refs): fp32 B_FMT[fmt] x max|lin| x GAIN (2e-6 H2, 4e-5 f8, 8e-5 f6; hi-only 5e-6 against the float64 product of
the f16-ROUNDED operands); hand-off of operand format i into container o: B_FMT[i] x max|lin| x GAIN x max(next style) + KEEP_FMT[o] x
max|want|, and for o = f8 the fp8(v / 4) plane within FP8_PLANE x max|want|.  Nothing new, nothing widened.

Observed on an MI355X, worst error / bound over every test of this file (the three forms of one operand format agree to the digits
shown; every run prints the figures per case):
    fp32       H2 0.24 (2.8e-6 of 1.1e-5)   f8 0.30 (9.6e-5 of 3.2e-4)   f6 0.18 (9.5e-5 of 5.3e-4)   hi-only 0.033 (1.1e-6 of 3.3e-5)
    -> H2      H2 0.16 (3.5e-6 of 2.1e-5)   f8 0.24 (9.2e-5 of 3.8e-4)   f6 0.15 (1.2e-4 of 7.9e-4)   hi-only 0.032 (1.7e-6 of 5.2e-5)
    -> f8      H2 0.57 (6.2e-5 of 1.1e-4)   f8 0.25 (1.4e-4 of 5.6e-4)   f6 0.15 (1.3e-4 of 8.9e-4)   hi-only 0.45 (6.1e-5 of 1.4e-4)
    fp8(v / 4) plane, every operand format: 0.80 ... 0.81 (0.250 of 0.309 ... 0.315)
(-> f8 from H2 / hi-only operands: the error IS the container's, 2e-5 of the largest value, the operands add next to nothing.)
No kernel had to be changed.  199 tests, 16 s."""
import ctypes
import functools

import pytest
import torch

import conv_form_refs as cf
from test_hip_conv_forms_f64 import _S, _check, _check_f32, _check_handoff, _dev_inputs, _lib, _noise_args, _packed, half_out, pinned
from test_hip_step_kernels import Out, P, U, within

pytestmark = pytest.mark.gpu

_LAUNCHED = {}                   # forms case that ran to its end -> (form, operand format, output 0 fp32 / 1 H2 / 2 f8)


def _run(lib, what, UP, fmt, route, r, nz_args, hooks):
    """One launch of nb_modconv3x3_up2_h3_ex under `hooks` through `route` (f32* / handoff-h2 / handoff-f8), checked against the
    reference r: fp32 into a NaN-filled buffer inside NaN guards; hand-off into c_next = c_next_of(c_out) channels with a style row
    stride of c_next + 8, the channel groups past c_out zero before and after, the guards NaN.  Returns the destination (`Out`)."""
    from brushstroke_engine_amd import ops
    n, ci, co, h, w = UP
    d, g = cf.inputs(2, *UP), _dev_inputs(2, *UP)
    xh, wp = _packed(2, *UP, 1 if fmt == 3 else fmt)               # (hi-only: the f8 operands, their corrections unused)
    dev = xh.device
    common = (P(g["dco"]),) + tuple(nz_args) + (P(g["bias"]),)
    tail = (n, h, w, co, cf.ALPHA, cf.GAIN, cf.CLAMP, _S())
    c_next = cf.c_next_of(co)
    o = {"handoff-h2": 0, "handoff-f8": 1}.get(route)
    with pinned(lib, **hooks):
        if o is None:
            dst = Out([n, co, 2 * h, 2 * w], dev)
            _check(lib.nb_modconv3x3_up2_h3_ex(P(xh), ci, P(wp), *common, P(dst.t), None, None, 0, 0, fmt, 0, *tail), what)
        else:
            dst = half_out(ops.h2_shape(n, c_next, 2 * h, 2 * w), dev, co // 8)
            _check(lib.nb_modconv3x3_up2_h3_ex(P(xh), ci, P(wp), *common, None, P(dst.t), P(g["nst"]), c_next + 8, c_next, fmt, o, *tail), what)
        torch.cuda.synchronize()
    if o is None:
        _check_f32(what, dst, r, cf.tol_f32(fmt, r["scale"]))
    else:
        want = cf.handoff_want(d, r["ref"], co)
        _check_handoff(what, dst, d, r, o, co, c_next, tol=cf.tol_handoff_x(fmt, o, r["scale"], d, want, co))
    return dst


def _form_hooks(form, **more):
    rows, persist = cf.UP2V_FORMS[form]
    return dict(up2_v2=1, up2v_rows=rows, up2v_persistent=persist, **more)


@pytest.mark.parametrize("form,fmt,shape,route", cf.up2v_cases(), ids=lambda v: str(v))
def test_up2v_forms_vs_float64(form, fmt, shape, route):
    """Every form x operand format x route on A (one chunk, ragged second slice, 13 rows = one tile), B (four chunks, two tile
    columns, 24 items: the renumbered order; all three noise modes), C (five chunks, three slices in co_ld 128, three tile rows; all
    three noise modes) and D (seven chunks, c_out 36: fp32 only, four tile columns, image shorter than a tile).  Operand format 2 is
    decoded by the H2 / f8 decoders like every other: the up=2 epilogue writes no f6.  Operand format 3 (the f8 packers' operands)
    is compared with the float64 product of the f16-rounded operands."""
    lib = _lib()
    UP = cf.UP2V_SHAPES[shape]
    n, ci, co, h, w = UP
    noise = cf.up2v_noise_mode(route)
    r = cf.reference(2, *UP, noise, hi=fmt == 3)
    what = f"up2v {form} {cf.FMT_NAME[fmt]} {shape} {route}"
    _run(lib, what, UP, fmt, route, r, _noise_args(_dev_inputs(2, *UP), noise, 4 * h * w), _form_hooks(form))
    _LAUNCHED[(form, fmt, shape, route)] = (form, fmt, {"handoff-h2": 1, "handoff-f8": 2}.get(route, 0))


def test_up2v_forms_launched_match_the_table():
    """The forms cases that passed in this process before this test are cases of the table, each launched as the instantiation
    the table names; where all of them ran -- a run of the whole file -- they reached all 36: 3 forms x 4 operand formats x 3 outputs."""
    cases = cf.up2v_cases()
    assert set(_LAUNCHED) <= set(cases)
    inst = set(_LAUNCHED.values())
    print(f"[conv-forms] up2v: {len(_LAUNCHED)} of {len(cases)} forms cases passed before this test, {len(inst)} of 36 instantiations")
    if len(_LAUNCHED) == len(cases):
        assert inst == {(form, fmt, o) for form in cf.UP2V_FORMS for fmt in cf.UP2V_FMTS for o in range(3)} and len(inst) == 36


@pytest.mark.parametrize("form,fmt,shape,route", cf.up2v_loop_cases(), ids=lambda v: str(v))
def test_up2v_tile_loop_vs_float64(form, fmt, shape, route):
    """The persistent kernel's SECOND iteration against float64: P1 (280 items: list and grid multiples of 8, the renumbered order, a
    second item in another sample) and P2 (282 items: the plain order, a second item in another sample AND another tile row or
    slice; every third tile one row high) at one persistent workgroup per CU (nb_debug_set_persistent_wgs_per_cu(1)): 256 workgroups,
    24 / 26 of them with a second item -- tile_coords, load_channel_tables and piece_sources again, the next tile's first chunk
    prefetched under the epilogue, noise tile and channel tables rewritten.  The one-workgroup-per-tile form walks the same item
    order on a grid of 280 / 282.  Fails, not skips, where the device has so many CUs that no workgroup gets a second item."""
    lib = _lib()
    UP = cf.UP2V_SHAPES[shape]
    n, ci, co, h, w = UP
    items = cf.up2v_geometry(shape, 12)[4]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert items > cus, f"{items} items on {cus} CUs: the tile loop would not be taken"
    r = cf.reference(2, *UP)
    what = f"up2v-loop {form} {cf.FMT_NAME[fmt]} {shape} {route} ({items} items, {cus} CUs)"
    _run(lib, what, UP, fmt, route, r, _noise_args(_dev_inputs(2, *UP), "per", 4 * h * w), _form_hooks(form, persistent_wgs_per_cu=1))


@functools.lru_cache(maxsize=None)
def _noise_tensors():
    """The noise of conv_form_refs.up2v_noise_case on the device: a one-layer nb_noise_f32 launch (the table of test_noise_vs_float64
    with one entry), once from the integer positions and once from their normalised form (nb_norm_positions_f32)."""
    from brushstroke_engine_amd import _lib as L
    lib = L.lib()
    c = cf.up2v_noise_case()
    dev = torch.device("cuda:0")
    n, res = c["pos"].shape[0], c["nc"].shape[0]
    t = {k: c[k].to(dev) for k in ("nc", "lin", "strength", "pos")}
    t["nc_t"] = t["nc"].t().contiguous()
    t["npos"] = torch.empty([n, 2], dtype=torch.float32, device=dev)
    L.check(lib.nb_norm_positions_f32(P(t["pos"]), cf.UP2V_NOISE_R, P(t["npos"]), n, _S()), "norm_positions")
    out = {}
    for form in ("positions", "norm_pos"):
        o = Out([n, res, res], dev)
        desc = (L.NbLayerDesc * 1)()
        desc[0].noise_const, desc[0].noise_lin, desc[0].noise_strength, desc[0].noise_out = P(t["nc"]), P(t["lin"]), P(t["strength"]), P(o.t)
        desc[0].res, desc[0].c_aff, desc[0].c_out, desc[0].style_scale = res, 3, 4, 1.0
        table = torch.frombuffer(bytearray(bytes(desc)), dtype=torch.uint8).to(dev)
        ip, fp = (t["pos"], None) if form == "positions" else (None, t["npos"])
        L.check(lib.nb_noise_f32(P(table), 1, res, P(fp), P(ip), cf.UP2V_NOISE_R, n, _S()), "noise")
        torch.cuda.synchronize()
        assert o.guards_untouched()
        out[form] = o.t
    assert torch.equal(t["npos"].cpu(), c["npos"])
    return t, out


@pytest.mark.parametrize("fmt", [0, 1])
@pytest.mark.parametrize("form", list(cf.UP2V_FORMS))
def test_up2v_noise_in_kernel(form, fmt):
    """Shape N (64 x 64 output, noise resolution 64, R = 256): the noise computed by the kernel itself (NbNoiseSrc: the constant
    transposed, the grid row, the strength; integer positions that are negative, beyond R and near +-2^40; then the same positions
    pre-normalised) against the launch reading the [n, 64, 64] tensor that nb_noise_f32 wrote from the same inputs: fp32 and hand-off
    destinations bit for bit, guards included.  At 13 rows the noise tile is written behind the K loop into the ring.  Both routes
    are also held to float64, with the device's noise tensor as the reference's noise (held to float64 itself by
    test_noise_vs_float64; here within 9 U x strength x max|constant| of the oracle's evaluation, the bound of that test with the
    four weights summed to 1)."""
    from brushstroke_engine_amd import _lib as L
    lib = _lib()
    UP = cf.UP2V_SHAPES["N"]
    n, ci, co, h, w = UP
    c = cf.up2v_noise_case()
    t, nz = _noise_tensors()
    assert torch.equal(nz["positions"].view(torch.int32), nz["norm_pos"].view(torch.int32))
    within(nz["positions"], cf.up2v_noise_ref(), 9 * U * float(c["strength"][0]) * float(c["nc"].abs().max()), "noise tensor vs oracle")
    lin, d = cf.linear(2, *UP), cf.inputs(2, *UP)
    pre, act, ref = cf.epilogue(lin, d, nz["positions"].cpu())
    r = dict(lin=lin, pre=pre, act=act, ref=ref, scale=float(lin.abs().max()) * cf.GAIN)
    assert not cf.blocks_meet_kink_and_clamp(pre, act, 2 * cf.UP2V_FORMS[form][0], 64, 32)
    for pos_form in ("positions", "norm_pos"):
        src = L.NbNoiseSrc(P(t["nc_t"]), P(t["lin"]), P(t["strength"]), P(t["npos"]) if pos_form == "norm_pos" else None,
                           P(t["pos"]) if pos_form == "positions" else None, 2 * h, cf.UP2V_NOISE_R)
        for route in ("f32", "handoff-" + cf.FMT_NAME[fmt]):
            what = f"up2v-noise {form} {cf.FMT_NAME[fmt]} N {route} {pos_form}"
            a = _run(lib, what + " tensor", UP, fmt, route, r, (P(nz[pos_form]), 4 * h * w), _form_hooks(form))
            b = _run(lib, what + " in-kernel", UP, fmt, route, r, (ctypes.addressof(src), L.NB_NOISE_IN_KERNEL), _form_hooks(form))
            bits = torch.int32 if a.buf.dtype == torch.float32 else torch.int16
            assert torch.equal(a.buf.view(bits), b.buf.view(bits)), f"{what}: in-kernel noise != noise tensor"


@pytest.mark.parametrize("shape,rows", [("S12", 12), ("S13", 13)])
def test_up2v_launcher_selection_vs_float64(shape, rows):
    """Every hook at its default: the launcher itself picks the kernel (nb_up2_h3_select), the tile height (nb_up2v_rows) and four
    persistent workgroups per CU.  First the library is asked what it will run -- a change of the selection fails here instead of
    silently running another kernel -- then the launch is held to float64, fp32 and f8 hand-off, f8 operands.  S12 is the smallest
    output at 16 -> <= 128 channels, w = 32 on which the selection is up2v with 12-row tiles (conv_form_refs.UP2V_SHAPES)."""
    lib = _lib()
    UP = cf.UP2V_SHAPES[shape]
    n, ci, co, h, w = UP
    lib.nb_debug_up2v_auto_rows.argtypes, lib.nb_debug_up2v_auto_rows.restype = [ctypes.c_int] * 5, ctypes.c_int
    with pinned(lib):
        pass                                                       # (every hook back to the library's own choice)
    buf = ctypes.create_string_buffer(64)
    _check(lib.nb_modconv3x3_up2_h3_variant(1, ci, co, n, h, w, buf, 64), "variant")
    assert buf.value.decode() == "modconv3x3_up2v_kernel", buf.value
    assert lib.nb_debug_up2v_auto_rows(ci, co, n, h, w) == rows
    r = cf.reference(2, *UP)
    for route in ("f32", "handoff-f8"):
        _run(lib, f"up2v-select {shape} f8 {route}", UP, 1, route, r, _noise_args(_dev_inputs(2, *UP), "per", 4 * h * w), {})


REFUSED = {
    # name -> (fmt, out_fmt, (n, ci, co, h, w), destinations: "f32" / "h2" / "none" / "both")
    "f6 operands on a shape up2v does not take (w = 16)": (2, 0, (2, 16, 32, 8, 16), "f32"),
    "out_fmt = 2": (1, 2, (1, 16, 32, 8, 32), "h2"),
    "f8 output with c_out % 16 != 0": (1, 1, (1, 16, 40, 8, 32), "h2"),
    "f8 operands with c_in % 16 != 0": (1, 0, (1, 24, 32, 8, 32), "f32"),
    "both destinations null": (1, 0, (1, 16, 32, 8, 32), "none"),
    "both destinations set": (1, 0, (1, 16, 32, 8, 32), "both"),
}


@pytest.mark.parametrize("case", list(REFUSED), ids=lambda v: v.replace(" ", "-"))
def test_up2v_refused_calls(case):
    """Calls the launcher must refuse: NB_EINVAL, and both NaN-filled destinations bitwise as they were.  (Every buffer has the size
    the call states, so a call that is wrongly accepted still stays inside its buffers.)"""
    from brushstroke_engine_amd import _lib as L
    from brushstroke_engine_amd import ops
    lib = _lib()
    fmt, out_fmt, UP, dst = REFUSED[case]
    n, ci, co, h, w = UP
    g = {k: v.cuda() for k, v in cf.inputs(2, *UP).items()}
    pack_x, pack_w = {1: (ops.pack_h2f8, ops.pack_conv_weight_h3f8), 2: (ops.pack_h2f6, ops.pack_conv_weight_h3f6)}[fmt]
    if ci % 16:
        pack_x, pack_w = ops.pack_h2, ops.pack_conv_weight_h3       # (only the container matters: the call is refused before anything reads it)
    xh, wp = pack_x(g["x"], g["st"]), pack_w(g["w"])
    c_next = cf.c_next_of(co)
    y = Out([n, co, 2 * h, 2 * w], xh.device)
    out = Out(ops.h2_shape(n, c_next, 2 * h, 2 * w), xh.device, dtype=torch.float16)
    before = y.buf.view(torch.int32).clone(), out.buf.view(torch.int16).clone()
    with pinned(lib, up2_v2=1):
        rc = lib.nb_modconv3x3_up2_h3_ex(P(xh), ci, P(wp), P(g["dco"]), P(g["noise"]), 4 * h * w, P(g["bias"]),
                                        P(y.t) if dst in ("f32", "both") else None, P(out.t) if dst in ("h2", "both") else None,
                                        P(g["nst"]), c_next + 8, c_next, fmt, out_fmt, n, h, w, co, cf.ALPHA, cf.GAIN, cf.CLAMP, _S())
        torch.cuda.synchronize()
    assert rc == L.NB_EINVAL, (case, rc)
    assert torch.equal(y.buf.view(torch.int32), before[0]) and torch.equal(out.buf.view(torch.int16), before[1]), f"{case}: destination written"
