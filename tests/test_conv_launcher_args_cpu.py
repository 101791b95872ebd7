"""The split-f16 conv launchers, the fp32 conv launchers (nb_modconv3x3_f32, nb_modconv3x3_up2_f32_h2, nb_modconv3x3_variant) and
the operand packers refuse bad calls on the host, before any launch: one table of bad calls, each with the NB_EINVAL it must return
and the text nb_last_error() must hold.  No GPU is needed -- no row gets as far as the zero page or a kernel.  The split-f16 up=1
and up=2 families share their launcher set-up (csrc/nb_h3_launch.h) but not every rule or text; rows that break two rules at once
pin the ORDER of the checks (the two families report a bad slope and a bad image size in opposite orders)."""
import ctypes

import pytest

from brushstroke_engine_amd import _lib, build

P = 0x100000          # a 16-byte aligned address that is never dereferenced
ODD = P + 4           # ... and a misaligned one

CONV = dict(x=P, c_in=64, wts=P, dcoefs=P, noise=None, nsn=0, bias=P, y=P, y_h2=None, next_styles=None, next_stride=0, c_next=0,
            t=None, in_fmt=0, out_fmt=0, n=2, h=64, w=64, c_out=64, alpha=0.2, gain=1.0, clamp=256.0, stream=None)
HANDOFF = dict(y=None, y_h2=P, next_styles=P, next_stride=64, c_next=64)
ORDER = {
    "_ex1": "x c_in wts dcoefs noise nsn bias y y_h2 next_styles next_stride c_next t in_fmt out_fmt n h w c_out alpha gain clamp stream",
    "_ex2": "x c_in wts dcoefs noise nsn bias y y_h2 next_styles next_stride c_next in_fmt out_fmt n h w c_out alpha gain clamp stream",
    "": "x c_in wts dcoefs noise nsn bias y n h w c_out alpha gain clamp stream",
    "_h2": "x c_in wts dcoefs noise nsn bias next_styles next_stride y_h2 c_next n h w c_out alpha gain clamp stream",
    "_torgb": "x c_in wts dcoefs noise nsn bias y n h w c_out alpha gain clamp t stream",
}


def torgb(**kw):
    d = dict(styles=P, w=P, bias=P, color_bias=P, styles_stride_n=64 + 9, render_mode=0, clamp=256.0)
    d.update(kw)
    return _lib.NbTorgbArgs(**d)


def conv(up, kind, **kw):
    """(entry name, argument tuple) of a conv call: the good call of that entry with `kw` changed."""
    d = dict(CONV)
    if kind == "_h2":
        d.update(HANDOFF)
    if kind == "_torgb":
        d["t"] = torgb()
    d.update(kw)
    t = d["t"]                # (returned with the call: the struct must outlive it)
    if isinstance(t, _lib.NbTorgbArgs):
        d["t"] = ctypes.addressof(t)
    order = ORDER[kind + str(up) if kind == "_ex" else kind].split()
    return f"nb_modconv3x3_up{up}_h3{kind}", tuple(d[k] for k in order), t


def rows():
    out = []

    def add(call, text):
        out.append(pytest.param(call, text, id=f"{call[0]}-{len(out)}"))
    for up in (1, 2):
        pre = f"modconv3x3_up{up}_h3: "
        size = "needs w % 32 == 0 and h % 16 == 0" if up == 1 else "needs w % 32 == 0, w == 16 or w == 8"
        for kind in ("_ex", "", "_h2") + (("_torgb",) if up == 1 else ()):
            add(conv(up, kind, x=None), pre + "null pointer")
            add(conv(up, kind, bias=None), pre + "null pointer")
            add(conv(up, kind, w=48), pre + size + " (got 64x48)")
            add(conv(up, kind, alpha=1.5), pre + "leaky-ReLU slope must lie in [0, 1] and the gain be positive (got 1.5, 1)")
            add(conv(up, kind, gain=0.0), pre + "leaky-ReLU slope must lie in [0, 1] and the gain be positive (got 0.2, 0)")
            add(conv(up, kind, x=ODD), pre + "pointers must be 16-byte aligned")
            add(conv(up, kind, wts=ODD), pre + "pointers must be 16-byte aligned")
            add(conv(up, kind, n=0), pre + "bad sizes")
            add(conv(up, kind, n=65536), pre + "bad sizes")
            # two rules broken at once: which one is reported
            add(conv(up, kind, alpha=1.5, w=48), pre + ("leaky-ReLU slope" if up == 1 else size + " (got 64x48)"))
            add(conv(up, kind, x=ODD, w=48), pre + size)
            add(conv(up, kind, x=None, w=48, n=0), pre + "null pointer")
            add(conv(up, kind, n=0, alpha=1.5), pre + "bad sizes")
            if up == 1:
                add(conv(up, kind, h=8), pre + size + " (got 8x64)")
            else:
                add(conv(up, kind, h=4), pre + size + " (got 4x64)")
        # operand and output formats (the _ex entries)
        f8 = "the f8 operand format needs c_in % 16 == 0 (got 24)" if up == 1 else "the f8 / f6 operand formats need c_in % 16 == 0 (got 24)"
        add(conv(up, "_ex", in_fmt=1, c_in=24), pre + f8)
        add(conv(up, "_ex", in_fmt=2, c_in=24), pre + f8)
        add(conv(up, "_ex", in_fmt=1, c_in=24, x=None), pre + ("null pointer" if up == 1 else f8))
        add(conv(up, "_ex", in_fmt=4), pre + ("operand format must be 0 (H2), 1 (f8), 2 (f6) or 3" if up == 1 else "input operand format must be 0 (H2), 1 (f8), 2 (f6) or 3"))
        add(conv(up, "_ex", out_fmt=1), pre + ("f8 / f6 output" if up == 1 else "f8 output") + " needs an H2 destination and c_out, c_next % 16 == 0")
        add(conv(up, "_ex", out_fmt=1, **dict(HANDOFF, c_next=72)), pre + ("f8 / f6 output" if up == 1 else "f8 output") + " needs an H2 destination")
        if up == 2:
            add(conv(up, "_ex", out_fmt=2, **HANDOFF), pre + "input operand format must be 0 (H2), 1 (f8), 2 (f6) or 3 (f8, hi only), output format 0 or 1 "
                "(the up=2 epilogue does not write the f6 format)")
        else:
            add(conv(up, "_ex", out_fmt=3, **HANDOFF), pre + "f8 / f6 output needs an H2 destination")
        # hand-off
        hand = pre + "H2 output needs the consumer's styles, c_out % 8 == 0 and c_next >= c_out"
        for kind in ("_ex", "_h2"):
            add(conv(up, kind, **dict(HANDOFF, c_next=32)), hand)
            add(conv(up, kind, **dict(HANDOFF, next_stride=32)), hand)
            add(conv(up, kind, **dict(HANDOFF, next_styles=None)), hand)
            add(conv(up, kind, **dict(HANDOFF, y_h2=ODD + 4)), hand)
            add(conv(up, kind, **dict(HANDOFF, c_next=60, next_stride=60), c_out=60), hand)
            add(conv(up, kind, **dict(HANDOFF, c_next=32), n=0, w=48), hand)
        add(conv(up, "_ex", **dict(HANDOFF, y=P)), pre + "null pointer")              # both outputs given
        add(conv(up, "_ex", y=None), pre + "null pointer")                            # ... and neither
        add(conv(up, "_h2", y_h2=None), pre + "null pointer")
    # fused ToRGB (up=1)
    for kind, name in (("_ex", "modconv3x3_up1_h3_ex"), ("_torgb", "modconv3x3_up1_h3_torgb")):
        cmax = name + ": the fused ToRGB needs all channels in one workgroup (c_out <= 128)"
        add(conv(1, kind, t=torgb(styles_stride_n=160 + 9), c_out=160), cmax)
        add(conv(1, kind, t=torgb(render_mode=2)), "Unknown render mode for TriadGanPaintEngine: 2")
        add(conv(1, kind, t=torgb(styles_stride_n=64 + 8)), "torgb_triad: styles rows must hold 9 color scalars + c styles")
        add(conv(1, kind, t=torgb(styles_stride_n=8, render_mode=2), c_out=160), cmax)
        add(conv(1, kind, t=torgb(styles_stride_n=8, render_mode=2)), "torgb_triad: styles rows must hold")
        add(conv(1, kind, t=torgb(styles=None)), name + (": bad ToRGB arguments" if kind == "_ex" else ": null pointer"))
        add(conv(1, kind, t=torgb(color_bias=None), c_out=160), name + (": bad ToRGB arguments" if kind == "_ex" else ": null pointer"))
        add(conv(1, kind, t=torgb(), w=48), "modconv3x3_up1_h3: needs w % 32 == 0 and h % 16 == 0 (got 64x48)")
        add(conv(1, kind, t=torgb(render_mode=2), x=None), "Unknown render mode")
    add(conv(1, "_ex", t=torgb(), **dict(HANDOFF, y=P)), "modconv3x3_up1_h3_ex: bad ToRGB arguments")
    add(conv(1, "_torgb", t=0), "modconv3x3_up1_h3_torgb: null pointer")
    # the activation packers
    for fmt in ("h2", "h2f8", "h2f6"):
        entry, bad = f"nb_pack_{fmt}_f32", f"pack_{fmt}: bad arguments"
        good = dict(x1=P, c1=32, x2=None, c2=0, scale=None, out=P, n=2, hw=4096, stream=None)
        for kw in (dict(x1=None), dict(out=None), dict(c1=0), dict(c2=16), dict(c2=-1), dict(n=0), dict(n=65536), dict(hw=0)):
            add((entry, tuple(dict(good, **kw).values())), bad)
        if fmt != "h2":
            add((entry, tuple(dict(good, c1=24).values())), f"pack_{fmt}: the {fmt[2:]} operand format needs a multiple of 16 channels (got 24)")
            add((entry, tuple(dict(good, c1=24, x2=P, c2=16).values())), f"pack_{fmt}: the {fmt[2:]} operand format needs a multiple of 16 channels (got 40)")
            add((entry, tuple(dict(good, c1=24, x1=None).values())), bad)
        entry, bad = f"nb_pack_{fmt}_part_f32", f"pack_{fmt}_part: bad arguments" + ("" if fmt == "h2" else " (whole 16-channel chunks only)")
        good = dict(x=P, c=32, scale=None, scale_stride=0, out=P, c8_total=8, cg0=2, n=2, hw=4096, stream=None)
        for kw in (dict(x=None), dict(out=None), dict(c=0), dict(n=0), dict(hw=0), dict(cg0=-2), dict(cg0=6)) + (() if fmt == "h2" else (dict(c=24), dict(cg0=1))):
            add((entry, tuple(dict(good, **kw).values())), bad)
    # the device weight packer
    good = dict(w=P, c_out=64, c_in=64, co_align=64, transpose_flip=0, out=P, stream=None)
    for kw in (dict(w=None), dict(out=None), dict(out=ODD), dict(c_out=0), dict(c_in=0), dict(co_align=32), dict(co_align=0)):
        add(("nb_pack_conv_weight_h3_dev", tuple(dict(good, **kw).values())), "pack_conv_weight_h3_dev: bad arguments")
    # the fp32 kernels (csrc/nb_modconv.hip): every rule stands before the zero page and the launch.  (New rows go to the END of the
    # table: a row's id carries its index.)
    f32 = dict(x1=P, c1=32, x2=None, c2=0, wpk=P, styles=P, dcoefs=P, noise=None, nsn=0, bias=P, out_scale=P, y=P, n=2, h=16, w=16, c_out=32,
               up=2, alpha=0.2, gain=1.0, clamp=256.0, stream=None)
    orders = {"nb_modconv3x3_f32": "x1 c1 x2 c2 wpk styles dcoefs noise nsn bias y n h w c_out up alpha gain clamp stream",
              "nb_modconv3x3_up2_f32_h2": "x1 c1 x2 c2 wpk styles dcoefs noise nsn bias out_scale y n h w c_out alpha gain clamp stream"}
    for entry, order in orders.items():
        call = lambda **kw: (entry, tuple(dict(f32, **kw)[k] for k in order.split()), None)
        for k in ("x1", "wpk", "styles", "dcoefs", "bias", "y"):
            add(call(**{k: None}), "modconv3x3: null pointer")
        add(call(c2=8), "modconv3x3: bad channel split c1=32 c2=8")
        add(call(c1=0), "modconv3x3: bad channel split c1=0 c2=0")
        add(call(c2=-1, x2=P), "modconv3x3: bad channel split c1=32 c2=-1")
        add(call(n=0), "modconv3x3: batch 0 out of range")
        add(call(n=65536), "modconv3x3: batch 65536 out of range")
        add(call(h=2), "modconv3x3: h,w must be powers of two >= 4 (got 2x16)")
        add(call(w=2), "modconv3x3: h,w must be powers of two >= 4 (got 16x2)")
        add(call(h=24), "modconv3x3: h,w must be powers of two >= 4 (got 24x16)")
        add(call(w=48), "modconv3x3: h,w must be powers of two >= 4 (got 16x48)")
        add(call(c_out=0), "modconv3x3: c_out=0")
        for k in ("x1", "wpk", "y"):
            add(call(**{k: ODD}), "modconv3x3: x1, x2, wpk and y must be 16-byte aligned")
        add(call(x2=ODD, c2=8), "modconv3x3: x1, x2, wpk and y must be 16-byte aligned")
        # two rules broken at once: the order of the checks
        add(call(x1=None, n=0), "modconv3x3: null pointer")
        add(call(n=0, w=48), "modconv3x3: batch 0 out of range")
        add(call(w=48, y=ODD), "modconv3x3: h,w must be powers of two")
    add(("nb_modconv3x3_f32", tuple(dict(f32, up=3)[k] for k in orders["nb_modconv3x3_f32"].split()), None), "modconv3x3: up=3 unsupported")
    add(("nb_modconv3x3_f32", tuple(dict(f32, up=0, y=ODD)[k] for k in orders["nb_modconv3x3_f32"].split()), None), "modconv3x3: up=0 unsupported")
    good = dict(n=2, h=16, w=16, c_out=32, up=1, buf=ctypes.create_string_buffer(64), buflen=64)
    for kw in (dict(buf=None), dict(buflen=0), dict(buflen=-1)):
        add(("nb_modconv3x3_variant", tuple(dict(good, **kw).values()), good["buf"]), "modconv3x3_variant: bad buffer")
    for kw in (dict(n=0), dict(h=2), dict(w=0), dict(c_out=0), dict(up=3), dict(up=0)):
        add(("nb_modconv3x3_variant", tuple(dict(good, **kw).values()), good["buf"]), "modconv3x3_variant: bad shape")
    return out


@pytest.fixture(scope="module")
def library():
    build.build()
    return _lib.lib()


@pytest.mark.parametrize("call, text", rows())
def test_bad_call_is_refused_with_its_message(library, call, text):
    entry, args = call[0], call[1]
    rc = getattr(library, entry)(*args)
    err = library.nb_last_error().decode()
    print(entry, rc, err)
    assert rc == _lib.NB_EINVAL, (entry, args, err)
    assert text in err, (entry, args, err)
