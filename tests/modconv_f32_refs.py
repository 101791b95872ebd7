"""The fp32-in / fp32-accumulate modulated 3 x 3 convolution (csrc/nb_modconv.hip: nb_modconv3x3_f32, nb_modconv3x3_up2_f32_h2): a
Python restatement of the launcher's kernel selection (nb_select_variant with the quad tile of the up = 2 kernels, the tile
geometry launch_up1 / launch_up2 derive from it), the case table of tests/test_hip_modconv_f32_f64.py -- every one of the 11
fp32-output kernels and the five H2OUT twins, each named with the kernel it must reach -- and the plain fp32 CPU evaluation that
shows the bound has room for another summation order.  TEST INFRASTRUCTURE: no GPU, no library call (tests/
test_modconv_f32_refs_cpu.py holds the restatement to the library's own answer).

Inputs, float64 reference, epilogue, mutations: tests/conv_form_refs.py (1.5-sized bias, unit noise, clamp 3.0 that is reached).
x is split into x1 / x2 by slicing.  The identity epilogue (alpha = 1, gain = 1, clamp = -1, zero bias, null noise: what the
training backward's role-swapped dx launch uses) has lin itself as its reference.

Bound: B_FMT[0] = 2e-6 of max|lin| x GAIN, elementwise -- what the hi / lo f16 kernels meet; fp32 operands with fp32 accumulation
may not be worse.  A plain fp32 evaluation on the CPU (torch float32 conv2d; conv_transpose2d + [1,3,3,1] FIR for up = 2) must
stay within a quarter of it on every case: a condition on the inputs."""
import collections
import functools

import torch

import conv_form_refs as cf

TARGET = 384                      # workgroups the selector wants on the chip
B = cf.B_FMT[0]
QUARTER = 0.25                    # the plain fp32 CPU evaluation must stay within this share of the bound

# selector index -> template arguments.  up = 1: modconv3x3_up1_kernel<NW, MB, NBW, KC, NST, SK>; up = 2: modconv3x3_up2_kernel<NBP, KC>
# (three ring stages: NB_UP2_STAGES)
UP1_KERNELS = {0: (8, 4, 1, 4, 3, False), 1: (8, 2, 2, 4, 3, False), 2: (4, 2, 2, 8, 4, False), 3: (4, 1, 2, 8, 4, False),
               4: (4, 1, 1, 8, 4, False), 10: (4, 1, 1, 8, 4, True)}
UP2_KERNELS = {5: (10, 4), 6: (6, 4), 7: (3, 8), 8: (2, 8), 9: (1, 8)}
UP2_STAGES = 3
UP2_TILES = ((16, 32), (16, 16), (8, 16), (8, 8), (4, 4))          # quad rows x columns per workgroup, in the selector's order
STY_MAX = 1024                                                     # NB_STY_MAX: the up = 2 kernels keep a sample's styles in LDS


def kernel_name(v):
    """What nb_modconv3x3_variant prints for selector index v."""
    if v in UP1_KERNELS:
        nw, mb, nbw, kc, nst, sk = UP1_KERNELS[v]
        return f"modconv3x3_up1_kernel<{nw}, {mb}, {nbw}, {kc}, {nst}, {'true' if sk else 'false'}>"
    return "modconv3x3_up2_kernel<%d, %d>" % UP2_KERNELS[v]


def kc_nst(v):
    """(input channels per chunk, ring stages) of selector index v."""
    return (UP1_KERNELS[v][3], UP1_KERNELS[v][4]) if v in UP1_KERNELS else (UP2_KERNELS[v][1], UP2_STAGES)


def up2_blocks(tqh, tqw):
    """16-position blocks per wave (NBP) that a quad tile with its one-quad halo needs on 4 waves."""
    return ((tqh + 2) * (tqw + 2) + 63) // 64


def select_variant(n, h, w, c_out, up):
    """nb_select_variant restated: (selector index, (quad rows, quad columns) of an up = 2 tile or None)."""
    if up == 1:
        cand = ((128, 256), (64, 512), (64, 256), (32, 256), (32, 128), (32, 32))      # c_out x pixels per workgroup (last: split-K)
        hw = h * w
        if hw <= 32:
            return 10, None
        best, best_wgs = 4, -1
        for i, (co_wg, pix) in enumerate(cand):
            if (i == 0 and c_out <= 64) or (i == 1 and (c_out <= 32 or c_out > 64)) or (i == 2 and c_out <= 32):
                continue
            wgs = n * ((hw + pix - 1) // pix) * ((c_out + co_wg - 1) // co_wg)
            v = 10 if i == 5 else i
            if wgs >= TARGET:
                return v, None
            if wgs > best_wgs:
                best_wgs, best = wgs, v
        return best, None
    best, best_wgs = 9, -1
    for th, tw in UP2_TILES:
        tqh, tqw = min(th, h), min(tw, w)
        nbp = up2_blocks(tqh, tqw)
        v = 5 if nbp > 6 else 6 if nbp > 3 else 7 if nbp > 2 else 8 if nbp > 1 else 9
        wgs = n * (h // tqh) * (w // tqw) * ((c_out + 15) // 16)
        if wgs >= TARGET:
            return v, (tqh, tqw)
        if wgs > best_wgs:
            best_wgs, best = wgs, v
    return best, (min(UP2_TILES[-1][0], h), min(UP2_TILES[-1][1], w))    # nothing reached the target: the smallest candidate's tile


def _up1_plane4(pix_wg):
    return max((pix_wg // 32 + 2) * 10, (min(pix_wg // 16, 16) + 2) * 6, (min(pix_wg // 8, 8) + 2) * 4, 6 * 3)


def up1_geometry(v, h, w):
    """launch_up1 restated: (tile width, tile rows, channels per workgroup, pixels per workgroup, fits): TW = min(w, 32),
    th = min(PIX_WG / TW, h); `fits` = the halo tile fits the kernel's LDS plane (the launcher refuses the call otherwise)."""
    nw, mb, nbw, kc, nst, sk = UP1_KERNELS[v]
    pix = (1 if sk else nw) * nbw * 32
    tw = min(w, 32)
    th = min(pix // tw, h)
    fits = (th + 2) * ((tw + 8) // 4) <= (_up1_plane4(pix) + 63) // 64 * 64
    return tw, th, 32 * mb, pix, fits


Case = collections.namedtuple("Case", "up n c1 c2 co h w noise epi variant tq")


def _c(up, n, c1, c2, co, h, w, noise, epi, variant, tq=None):
    return Case(up, n, c1, c2, co, h, w, noise, epi, variant, tq)


# Two shapes per kernel, as few outputs as the selector lets that kernel have, each shape shared by two cases (one float64 lin):
#   S1  ragged last slice, >= 2 slices and >= 2 tiles each way (where the selector allows it), more chunks than ring stages, c_in
#       no multiple of KC:  a  per-sample noise, live epilogue, a second input behind a first one with c1 % 4 != 0
#                           d  the identity epilogue of the backward's dx launch (null noise), c1 % 4 == 0
#   S2  ONE chunk (c_in < KC); up = 1: an image narrower than 32 and, where the selector allows it, shorter than the tile;
#       up = 2: a quad tile clipped by h or w where one selects the kernel:
#                           b  shared noise, no second input     c  null noise with the live bias, a second input
# one more case for every other clipped geometry that reaches the kernel, and per kernel
#   L   a long K loop, c_in = 101 + 28 = 129 (up = 2: 53 + 12 = 65, beyond which the plain fp32 conv_transpose2d + FIR of the CPU has no
#       quarter of the bound left): 17 / 9 chunks of 8 or 33 / 17 of 4, the ring gone round many times, on the smallest shape that
#       reaches the kernel (the error of one fp32 accumulator grows with the length of its chain: docs/kernel_notes.md)
CASES = [
    # ---- up = 1 ----------------------------------------------------------------------------------------------------------
    _c(1, 3, 9, 4, 136, 64, 256, "per", "live", 0),       # 8 x 32 tiles: 8 x 8 of them; slices 128 + 8 (wpk rows read past c_out_ld)
    _c(1, 3, 8, 5, 136, 64, 256, "null", "identity", 0),
    _c(1, 192, 3, 0, 136, 8, 8, "shared", "live", 0),     # TW = 8, th = 8 of 32
    _c(1, 192, 2, 1, 136, 8, 8, "null", "live", 0),
    _c(1, 192, 101, 28, 136, 8, 8, "per", "live", 0),
    _c(1, 12, 9, 4, 36, 64, 256, "per", "live", 1),       # 16 x 32 tiles: 4 x 8; one slice of 64 is all the selector gives this kernel
    _c(1, 12, 8, 5, 36, 64, 256, "null", "identity", 1),
    _c(1, 384, 3, 0, 40, 8, 8, "shared", "live", 1),      # TW = 8, th = 8 of 64
    _c(1, 384, 2, 1, 40, 8, 8, "null", "live", 1),
    _c(1, 384, 101, 28, 40, 8, 8, "per", "live", 1),
    _c(1, 3, 29, 6, 72, 64, 256, "per", "live", 2),       # 8 x 32 tiles, slices 64 + 8; 5 chunks of 8 on a ring of 4
    _c(1, 3, 32, 3, 72, 64, 256, "null", "identity", 2),
    _c(1, 192, 7, 0, 72, 8, 8, "shared", "live", 2),      # TW = 8, th = 8 of 32
    _c(1, 192, 4, 3, 72, 8, 8, "null", "live", 2),
    _c(1, 192, 101, 28, 72, 8, 8, "per", "live", 2),
    _c(1, 3, 29, 6, 36, 64, 256, "per", "live", 3),       # 8 x 32 tiles, slices 32 + 4
    _c(1, 3, 32, 3, 36, 64, 256, "null", "identity", 3),
    _c(1, 384, 7, 0, 8, 8, 8, "shared", "live", 3),       # TW = 8, th = 8 of 32
    _c(1, 384, 4, 3, 8, 8, 8, "null", "live", 3),
    _c(1, 384, 101, 28, 8, 8, 8, "per", "live", 3),
    _c(1, 3, 29, 6, 36, 32, 256, "per", "live", 4),       # 4 x 32 tiles: 8 x 8
    _c(1, 3, 32, 3, 36, 32, 256, "null", "identity", 4),
    _c(1, 192, 7, 0, 8, 16, 16, "shared", "live", 4),     # TW = 16, th = 8: two tile rows (no shape with a clipped tile selects this kernel)
    _c(1, 192, 4, 3, 8, 16, 16, "null", "live", 4),
    _c(1, 192, 101, 28, 8, 16, 16, "per", "live", 4),
    _c(1, 1, 29, 6, 72, 8, 64, "per", "live", 10),        # split-K: 1 x 32 tiles, 8 x 2 of them; 3 slices
    _c(1, 1, 32, 3, 72, 8, 64, "null", "identity", 10),
    _c(1, 1, 101, 28, 72, 8, 64, "per", "live", 10),
    _c(1, 2, 7, 0, 24, 4, 4, "shared", "live", 10),       # TW = 4, th = 4 of 8: half the workgroup's pixels lie below the image
    _c(1, 2, 4, 3, 24, 4, 4, "null", "live", 10),
    _c(1, 3, 29, 6, 72, 4, 8, "per", "live", 10),         # TW = 8: 4 x 8 in one workgroup
    _c(1, 5, 8, 6, 8, 8, 4, "shared", "live", 10),        # TW = 4, th = 8
    _c(1, 200, 9, 2, 24, 8, 8, "null", "identity", 10),   # (reached as the selector's last candidate, not as its fall-back)
    # ---- up = 2 ----------------------------------------------------------------------------------------------------------
    _c(2, 6, 9, 4, 20, 128, 128, "per", "live", 5, (16, 32)),     # 8 x 4 tiles, slices 16 + 4; 4 chunks of 4 on a ring of 3
    _c(2, 6, 8, 5, 20, 128, 128, "null", "identity", 5, (16, 32)),
    _c(2, 12, 3, 0, 8, 64, 256, "shared", "live", 5, (16, 32)),   # (no clipped tile selects this kernel: 16 x 32 quads only)
    _c(2, 12, 2, 1, 8, 64, 256, "null", "live", 5, (16, 32)),
    _c(2, 12, 53, 12, 8, 64, 256, "per", "live", 5, (16, 32)),
    _c(2, 3, 9, 4, 20, 128, 128, "per", "live", 6, (16, 16)),
    _c(2, 3, 8, 5, 20, 128, 128, "null", "identity", 6, (16, 16)),
    _c(2, 96, 3, 0, 24, 4, 64, "shared", "live", 6, (4, 32)),     # clipped by h
    _c(2, 96, 2, 1, 24, 4, 64, "null", "live", 6, (4, 32)),
    _c(2, 96, 53, 12, 24, 4, 64, "per", "live", 6, (4, 32)),
    _c(2, 192, 4, 2, 20, 8, 32, "per", "live", 6, (8, 32)),
    _c(2, 3, 29, 6, 20, 64, 128, "per", "live", 7, (8, 16)),      # 8 x 8 tiles; 5 chunks of 8 on a ring of 3
    _c(2, 3, 32, 3, 20, 64, 128, "null", "identity", 7, (8, 16)),
    _c(2, 64, 7, 0, 40, 32, 8, "shared", "live", 7, (16, 8)),     # clipped by w
    _c(2, 64, 4, 3, 40, 32, 8, "null", "live", 7, (16, 8)),
    _c(2, 64, 53, 12, 40, 32, 8, "per", "live", 7, (16, 8)),
    _c(2, 3, 29, 6, 20, 64, 64, "per", "live", 8, (8, 8)),
    _c(2, 3, 32, 3, 20, 64, 64, "null", "identity", 8, (8, 8)),
    _c(2, 64, 7, 0, 40, 4, 32, "shared", "live", 8, (4, 16)),     # clipped by h
    _c(2, 64, 4, 3, 40, 4, 32, "null", "live", 8, (4, 16)),
    _c(2, 64, 53, 12, 40, 4, 32, "per", "live", 8, (4, 16)),
    _c(2, 96, 9, 5, 20, 32, 4, "per", "live", 8, (16, 4)),        # clipped by w
    _c(2, 3, 29, 6, 72, 8, 8, "per", "live", 9, (4, 4)),          # 2 x 2 tiles, 5 slices
    _c(2, 3, 32, 3, 72, 8, 8, "null", "identity", 9, (4, 4)),
    _c(2, 3, 53, 12, 72, 8, 8, "per", "live", 9, (4, 4)),
    _c(2, 2, 7, 0, 40, 4, 4, "shared", "live", 9, (4, 4)),
    _c(2, 2, 4, 3, 40, 4, 4, "null", "live", 9, (4, 4)),
    _c(2, 48, 8, 6, 18, 4, 32, "per", "live", 9, (4, 8)),         # 4 x 8 quads: twice the noise tile of the square 4 x 4 ...
    _c(2, 48, 7, 0, 22, 32, 4, "shared", "live", 9, (8, 4)),      # ... and 8 x 4
]


def case_id(c):
    return f"up{c.up}-v{c.variant}-n{c.n}-{c.c1}+{c.c2}-{c.co}-{c.h}x{c.w}-{c.noise}-{c.epi}"


def shape_of(c):
    """The key of conv_form_refs.inputs / linear / reference."""
    return c.up, c.n, c.c1 + c.c2, c.co, c.h, c.w


def block_of(c):
    """(output rows, output columns, channels) of one workgroup's block of outputs."""
    if c.up == 1:
        tw, th, co_wg, pix, fits = up1_geometry(c.variant, c.h, c.w)
        return th, tw, co_wg
    return 2 * c.tq[0], 2 * c.tq[1], 16


def tiles_of(c):
    """(tile rows, tile columns, channel slices) of a launch."""
    th, tw, cs = block_of(c)
    return c.up * c.h // th, c.up * c.w // tw, (c.co + cs - 1) // cs


def h2_allowed(c):
    """The cases that also run through nb_modconv3x3_up2_f32_h2: every up = 2 case.  The launcher has no rule on c_out; the kernel
    writes whole groups of 4 channels (zeros behind c_out) into ceil(c_out / 8) groups of 8."""
    return c.up == 2


def epilogue_args(c):
    """(alpha, gain, clamp) of the launch."""
    return (cf.ALPHA, cf.GAIN, cf.CLAMP) if c.epi == "live" else (1.0, 1.0, -1.0)


def reference(c):
    """dict(lin, pre, act, ref, scale = max|lin| x GAIN) in float64.  Identity epilogue: ref = lin; the scale of its bound is the
    table-wide max|lin| x GAIN all the same (GAIN = sqrt 2 of the live cases, although the launch's own gain is 1): without a clamp
    that hides the largest outputs the plain fp32 evaluation of these cases lies at 4.2e-7 .. 5.4e-7 of max|lin|, which is no
    quarter of 2e-6 any more, and a bound that the yardstick itself leaves no room under says nothing about a kernel."""
    if c.epi == "live":
        return cf.reference(*shape_of(c), c.noise)
    lin = cf.linear(*shape_of(c))
    return dict(lin=lin, pre=lin, act=lin, ref=lin, scale=float(lin.abs().max()) * cf.GAIN)


@functools.lru_cache(maxsize=None)
def linear_f32(up, n, ci, co, h, w):
    """The same lin in plain fp32 on the CPU: float32 conv2d (up = 1); float32 conv_transpose2d + the [1,3,3,1] FIR (up = 2)."""
    from oracle import neube_oracle as orc
    d = cf.inputs(up, n, ci, co, h, w)
    xm = d["x"] * d["st"][:, :, None, None]
    if up == 1:
        lin = torch.nn.functional.conv2d(xm, d["w"], padding=1)
    else:
        lin = orc.conv2d_resample(xm, d["w"], f=orc.setup_filter([1, 3, 3, 1]), up=2, padding=1, flip_weight=False)
    assert lin.dtype == torch.float32
    return lin * d["dco"][:, :, None, None]


def evaluate_f32(c):
    """The whole layer in plain fp32 on the CPU, epilogue included (the order of the kernel's nb_epilogue)."""
    d = cf.inputs(*shape_of(c))
    lin = linear_f32(*shape_of(c))
    if c.epi != "live":
        return lin
    v = lin
    if c.noise != "null":
        v = v + (d["noise"][:, None] if c.noise == "per" else d["noise"][:1, None])
    v = v + d["bias"][None, :, None, None]
    v = torch.where(v < 0, v * cf.ALPHA, v) * cf.GAIN
    return v.clamp(-cf.CLAMP, cf.CLAMP)


def identity_mutations(c):
    """name -> mutated reference of an identity-epilogue case (no noise, bias, kink or clamp to get wrong)."""
    up, n, ci, co, h, w = shape_of(c)
    d, lin = cf.inputs(up, n, ci, co, h, w), cf.linear(up, n, ci, co, h, w)
    from test_hip_f8 import _conv_ref
    out = {}
    k = ci // 2
    out["input channel zeroed"] = lin - _conv_ref(d["x"][:, k:k + 1], d["w"][:, k:k + 1], d["st"][:, k:k + 1], up) * d["dco"].double()[:, :, None, None]
    m = lin.clone()
    rows = min(max(block_of(c)[0], 2), lin.shape[2])
    m[:, :, :rows] = torch.roll(lin[:, :, :rows], 1, dims=2)
    out["row shifted inside a tile"] = m
    m = lin.clone()
    m[:, co - (co % 8 or 8):] = 0
    out["last c_out group zeroed"] = m
    out["the live epilogue's slope and gain"] = torch.where(lin >= 0, lin, cf.ALPHA * lin) * cf.GAIN
    return out
