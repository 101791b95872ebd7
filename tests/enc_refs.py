"""float64 restatement of the geometry encoder's kernels (csrc/nb_encoder.hip) -- the 3 x 3 layer on the large tiles through every
output route, the same layer on the 32-position split-K tiles, the 7 x 7 stem, the bilinear x 2 -- with the decoders of the operand
containers they write, the bounds, the seeded inputs and the case tables of tests/test_hip_enc_routes_f64.py, and the mutated
references that tests/test_enc_refs_cpu.py uses to show that these cases can tell a wrong kernel from a right one.
TEST INFRASTRUCTURE: no GPU, no library call; plain torch on the CPU, float64 (the bilinear's sample coordinates alone are fp32,
because PyTorch and the kernel compute them so).

References
    conv_ref      lin = cross-correlation of the reflect-padded (1) input, before the bias;  out = lrelu(lin + b) * oscale[n, co]
    stem_ref      preprocessing 0 / 1 / 2 of autoenc/base.py (x, (1 - x) 2 - 1, 1 - x), reflect padding 3, 7 x 7, bias, lrelu
    upsample_ref  bilinear x 2, align_corners=True: s = float(h - 1) / float(2 h - 1), f = s * o, i0 = int(f), l = f - i0, 1 - l in
                  fp32 (each of these operations is one correctly rounded fp32 operation in the kernel: the library is built without
                  contraction), the four-term blend hy (hx a + lx b) + ly (hx c + lx d) in float64

Bounds, all from the project (conv_form_refs: B_FMT, KEEP_FMT, FP8_PLANE, CATCH)
    fp32 output      B_FMT[in_fmt] x max|lin| x max(1, max|oscale|)      (bias, lrelu: 1-Lipschitz behind the linear output)
    decoded operand  that + KEEP_FMT[out_fmt] x max|want|                 (H2: hi + lo; f8: hi + fp8(xl 2^9) / 512)
    fp8(v / 4) plane FP8_PLANE x max|want|
    stem             STEM_B x max|lin| (+ what the container keeps), STEM_B = B_FMT[0]
    bilinear         UP_B x max|x| (+ what the container keeps).  The coordinates and weights are the reference's own, so what is
                     left are the fp32 roundings of the blend: p = fl(hx a), q = fl(lx b) (errors <= u hx |a|, u lx |b|, u = 2^-24),
                     r = fl(p + q) (<= u |p + q|): the inner sum carries <= 2 u (hx + lx) max|x|; fl(hy r) adds u hy max|x|, likewise
                     ly; the final addition adds u max|x|.  With hx + lx = hy + ly = 1 (to 2^-25): 2 u + u + u = 4 u max|x|; second-
                     order terms are below 2^-20 of that.  UP_B = 4 x 2^-24 x (1 + 2^-20)."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from conv_form_refs import B_FMT, CATCH, FP8_PLANE, KEEP_FMT          # noqa: F401  (re-exported: the tests take them from here)

SLOPE = 0.01
N_CONV = 3                                            # samples of every conv case
# the stem's 49-term split-f16 sum, relative to max|lin|: the generator kernels' own bound.  Observed on an MI355X over the six (size,
# preprocessing) cases of STEM with H2 output: 2.1e-7 ... 2.9e-7, so the bound holds as it is and no measured constant takes its place
STEM_B = B_FMT[0]
UP_B = 4 * 2.0 ** -24 * (1 + 2.0 ** -20)              # bilinear: four fp32 roundings on the value path (docstring)
CO_WG = 128                                           # c_out channels of one large-tile workgroup
SMALL_CO = 32                                         # ... of one split-K workgroup
TILE = {"wide": (8, 32), "narrow": (16, 16)}         # output rows x columns of a large tile (LW = 5 / 4)
OSC_PAD, OSC_OFF = 24, 8                              # oscale rows are c_out + OSC_PAD long; the pointer starts OSC_OFF into the first


# ---------------------------------------------------------------------------------------------------------------------
# case tables
# ---------------------------------------------------------------------------------------------------------------------

# route -> (out_fmt: None fp32 | 0 H2 | 1 f8, windowed, scaled).  Windowed: channel groups cg0 = 2 .. of a consumer tensor with
# c8_total = cg0 + c_out / 8 + 2 groups.  Plain f8 passes c8_total = c_out / 8, plain H2 c8_total = 0, as encoder.py does.
ROUTES = {"f32": (None, False, False), "h2": (0, False, False), "f8": (1, False, False), "win-h2": (0, True, False),
          "win-f8": (1, True, False), "win-h2-osc": (0, True, True), "win-f8-osc": (1, True, True)}
ALL = tuple(ROUTES)
WIN_CG0, WIN_EXTRA = 2, 2

# Large tiles: (stride, tile, in_fmt, c_in, c_out, (out rows, out columns), routes); "@" behind a route = through
# nb_enc_conv3x3_h3_handoff itself (H2 operands), everything else through nb_enc_conv3x3_ex.  Sizes: one tile (8 x 32 / 16 x 16) or
# 2 x 2 and 2 x 3 tiles (16 x 64 / 32 x 48: 48 is the R = 384 width).  c_in 16 = one chunk (f8 loop: the third tap's pairing has no
# next step), 48 = an odd chunk count, 40 = a half-filled last chunk (H2 operands only).  c_out 144 = a second, ragged 128-slice,
# 20 = fp32 only, 24 = whole 8-channel groups but half a 16-channel chunk (H2 containers only).
LARGE = [
    (1, "wide", 0, 16, 144, (16, 64), ALL),
    (1, "wide", 0, 40, 20, (8, 32), ("f32",)),
    (1, "wide", 0, 64, 24, (8, 32), ("h2", "win-h2")),
    (1, "narrow", 0, 48, 48, (32, 48), ALL),
    (1, "narrow", 0, 64, 16, (16, 16), ("f32", "win-h2-osc@", "win-f8-osc@")),
    (2, "wide", 0, 64, 48, (8, 32), ("f32", "h2", "win-h2-osc@", "win-f8-osc@")),
    (2, "wide", 0, 48, 16, (16, 64), ("f32", "f8", "win-h2", "win-f8")),
    (2, "narrow", 0, 40, 144, (32, 48), ("f32", "h2", "f8", "win-h2-osc", "win-f8-osc")),
    (2, "narrow", 0, 16, 20, (16, 16), ("f32",)),
    (2, "narrow", 0, 16, 24, (16, 16), ("h2", "win-h2")),
    (1, "wide", 1, 16, 48, (16, 64), ALL),
    (1, "wide", 1, 64, 20, (8, 32), ("f32",)),
    (1, "narrow", 1, 48, 144, (32, 48), ALL),
    (1, "narrow", 1, 16, 16, (16, 16), ("f32", "f8")),
    (2, "wide", 1, 48, 144, (16, 64), ALL),
    (2, "wide", 1, 16, 16, (8, 32), ("f32", "h2", "win-f8-osc")),
    (2, "wide", 1, 64, 48, (8, 32), ("f32", "f8")),
    (2, "narrow", 1, 64, 48, (32, 48), ALL),
    (2, "narrow", 1, 16, 144, (16, 16), ("f32", "win-h2-osc")),
    (2, "narrow", 1, 48, 20, (16, 16), ("f32",)),
]


def large_cases():
    """[(stride, tile, in_fmt, c_in, c_out, ho, wo, route, api)], api = "ex" | "handoff"."""
    out = []
    for stride, tile, in_fmt, ci, co, (ho, wo), routes in LARGE:
        for r in routes:
            out.append((stride, tile, in_fmt, ci, co, ho, wo, r.rstrip("@"), "handoff" if r.endswith("@") else "ex"))
    return out


def launcher_tile(ho, wo):
    """The tile nb_enc_conv3x3_impl picks for an output size (None: the large tiles cannot take it)."""
    if wo % 32 == 0 and ho % 8 == 0:
        return "wide"
    return "narrow" if wo % 16 == 0 and ho % 16 == 0 else None


def instantiation(stride, tile, in_fmt, route):
    """<STRIDE, LW, OUT, F8> of enc_conv3x3_h3_kernel that a large case runs."""
    return stride, 5 if tile == "wide" else 4, 0 if route == "f32" else 1, bool(in_fmt)


# Small tiles (nb_debug_set_enc_small(1); H2 operands): (stride, c_in, c_out, out rows, out columns, route).  4 x 4 outputs: half of
# the 8-row tile is masked; 6 x 8: two tile rows, the second half masked; c_in 16: three of the four K-split waves own no chunk;
# c_out 40: a ragged 32-slice (fp32); 8 x 32 at stride 2: the 32-wide, one-row tile.
SMALL = [
    (1, 16, 8, 4, 4, "f32"), (1, 16, 8, 4, 4, "h2"), (2, 48, 40, 4, 4, "f32"), (2, 256, 64, 4, 4, "h2"),
    (1, 48, 64, 8, 8, "h2"), (1, 256, 40, 8, 8, "f32"), (2, 16, 64, 8, 8, "f32"),
    (1, 48, 40, 6, 8, "f32"), (2, 16, 8, 6, 8, "h2"),
    (1, 256, 8, 16, 16, "f32"), (1, 16, 64, 16, 16, "h2"), (2, 48, 40, 16, 16, "f32"),
    (2, 16, 8, 8, 32, "h2"), (2, 256, 64, 8, 32, "f32"), (2, 48, 40, 8, 32, "f32"),
]


def small_tile(wo):
    """(rows, columns) of a split-K tile's 32 positions."""
    cols = 32 if wo >= 32 else wo
    return 32 // cols, cols


# Stem: (n, h, w, preproc, out_fmt); 16 x 32 is a single tile with all four reflections in one workgroup
STEM = [(2, h, w, pre, fmt) for (h, w) in ((16, 32), (32, 64)) for pre in (0, 1, 2) for fmt in (0, 1)]

# Bilinear: (n, c, h, w, out_fmt, sampled).  (3, 16, 512, 512): 6.3 M work items on the 16384 x 256 grid cap (the strided loop runs
# twice for half of the threads); compared at sampled positions to keep the float64 reference small.
UPSAMPLE = [(2, 16, 2, 2, 0, False), (2, 16, 2, 2, 1, False), (1, 8, 5, 3, 0, False), (2, 32, 16, 32, 0, False),
            (2, 32, 16, 32, 1, False), (3, 16, 512, 512, 1, True)]
UP_GRID_CAP = 16384 * 256
UP_SAMPLES = 1 << 16


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------

# cases whose first seed leaves a block short of the kink, or a sample's oscale of one sign (tests/test_enc_refs_cpu.py says which):
# the next seed that does not
SEED_SALT = {}


def seed_of(*key):
    s = 7
    for k in key:
        s = (s * 1000003 + int(k) + 17) % (2 ** 31 - 1)
    return (s + 104729 * SEED_SALT.get(tuple(key), 0)) % (2 ** 31 - 1)


def _f(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


@functools.lru_cache(maxsize=None)
def conv_inputs(kind, stride, ci, co, ho, wo):
    """Seeded fp32 inputs of one 3 x 3 layer (kind 0 large tiles, 1 small): x randn, w randn / sqrt(9 c_in), b randn; osc_buf = the
    flat buffer the output scales live in (rows of c_out + OSC_PAD, both signs, |s| in [0.5, 1.5]); the kernel gets
    osc_buf + OSC_OFF with oscale_stride = c_out + OSC_PAD, so sample k's scales are osc_buf[OSC_OFF + k stride + co]."""
    rs = np.random.RandomState(seed_of(kind, stride, ci, co, ho, wo))
    n, ost = N_CONV, co + OSC_PAD
    buf = rs.uniform(0.5, 1.5, n * ost + OSC_OFF) * rs.choice([-1.0, 1.0], n * ost + OSC_OFF)
    return dict(x=_f(rs.randn(n, ci, stride * ho, stride * wo)), w=_f(rs.randn(co, ci, 3, 3) / np.sqrt(9 * ci)), b=_f(rs.randn(co)),
                osc_buf=_f(buf), ostride=ost)


def oscale_of(d, co, row_stride=None):
    """[n, c_out] scales as the kernel reads them (row_stride: the MUTATION `rows read with stride c_out`)."""
    st = d["ostride"] if row_stride is None else row_stride
    return torch.stack([d["osc_buf"][OSC_OFF + k * st:OSC_OFF + k * st + co] for k in range(N_CONV)])


@functools.lru_cache(maxsize=None)
def stem_inputs(n, h, w):
    """Image in [0, 1] with exact 0, exact 1 and grays (a thresholded drawing with gray rows, as the engine sees it); w randn / 7."""
    rs = np.random.RandomState(seed_of(2, n, h, w))
    x = (rs.rand(n, 1, h, w) > 0.3).astype(np.float32)
    x[:, :, ::3, :] = rs.rand(n, 1, len(range(0, h, 3)), w)
    x[:, :, 1, :4] = [0.0, 1.0, 0.5, 0.25]
    return dict(x=_f(x), w=_f(rs.randn(64, 1, 7, 7) / 7), b=_f(rs.randn(64)))


@functools.lru_cache(maxsize=None)
def upsample_input(n, c, h, w):
    return _f(np.random.RandomState(seed_of(3, n, c, h, w)).randn(n, c, h, w))


# ---------------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------------

def lrelu(t, slope=SLOPE):
    return torch.where(t >= 0, t, slope * t)


def _lin(x, w, stride, pad_mode="reflect", even_window=False):
    """Cross-correlation in float64.  even_window: the MUTATION `the stride-2 window starts at 2 i` (taps 2 i .. 2 i + 2: the
    kernel's shift form on a padded layer), else at 2 i - 1."""
    pad = (0, 1, 0, 1) if even_window else (1, 1, 1, 1)
    return F.conv2d(F.pad(x.double(), pad, mode=pad_mode), w.double(), stride=stride)


def conv_ref(x, w, b, stride, slope=SLOPE, oscale=None):
    """(lin, out): lin = reflect-padded (1) cross-correlation before the bias; out = lrelu(lin + b) * oscale[n, co]."""
    lin = _lin(x, w, stride)
    return lin, finish(lin, b, slope, oscale)


def finish(lin, b, slope=SLOPE, oscale=None):
    out = lrelu(lin + b.double()[None, :, None, None], slope)
    return out if oscale is None else out * oscale.double()[:, :, None, None]


@functools.lru_cache(maxsize=None)
def conv_lin(kind, stride, ci, co, ho, wo):
    """One float64 lin per shape, shared by every route and test of the shape, never written to."""
    d = conv_inputs(kind, stride, ci, co, ho, wo)
    return _lin(d["x"], d["w"], stride)


def conv_want(kind, stride, ci, co, ho, wo, route):
    """(lin, want, oscale or None) of a case's route."""
    d = conv_inputs(kind, stride, ci, co, ho, wo)
    osc = oscale_of(d, co) if ROUTES[route][2] else None
    lin = conv_lin(kind, stride, ci, co, ho, wo)
    return lin, finish(lin, d["b"], SLOPE, osc), osc


def preprocess(x, preproc):
    x = x.double()
    return (1 - x) * 2 - 1 if preproc == 1 else 1 - x if preproc == 2 else x


def stem_ref(x, w, b, preproc, slope=SLOPE, transposed=False):
    """(lin, out) of the stem.  transposed: the MUTATION `taps transposed`."""
    wd = w.double().transpose(2, 3) if transposed else w.double()
    lin = F.conv2d(F.pad(preprocess(x, preproc), (3, 3, 3, 3), mode="reflect"), wd)
    return lin, lrelu(lin + b.double()[None, :, None, None], slope)


def up_axis(size, other=None, align=True):
    """fp32 sample coordinates of one axis of the x 2 bilinear, as PyTorch and the kernel compute them: (i0, i1, l, 1 - l) for the
    2 size outputs.  other: the MUTATION `h and w swapped in the scale`; align=False: the MUTATION `align_corners=False`."""
    f32 = torch.float32
    o = torch.arange(2 * size, dtype=f32)
    if align:
        s_of = size if other is None else other
        s = torch.tensor(float(s_of - 1), dtype=f32) / torch.tensor(float(2 * s_of - 1), dtype=f32)
        f = s * o
    else:
        f = ((o + 0.5) * 0.5 - 0.5).clamp(min=0)
    i0 = f.to(torch.int64).clamp(max=size - 1)
    i1 = i0 + (i0 < size - 1).to(torch.int64)
    lam = f - i0.to(f32)
    return i0, i1, lam.double(), (1 - lam).double()


def upsample_ref(x, swap=False, align=True):
    """Bilinear x 2, align_corners=True: fp32 coordinates, float64 blend (module docstring)."""
    n, c, h, w = x.shape
    y0, y1, ly, hy = up_axis(h, w if swap else None, align)
    x0, x1, lx, hx = up_axis(w, h if swap else None, align)
    xd = x.double()
    top, bot = xd[:, :, y0], xd[:, :, y1]
    a, b_, c_, d_ = top[..., x0], top[..., x1], bot[..., x0], bot[..., x1]
    return hy[:, None] * (hx * a + lx * b_) + ly[:, None] * (hx * c_ + lx * d_)


def upsample_ref_at(x, ns, oys, oxs, align=True):
    """The same at sampled output positions: [K, c] for index vectors (sample, output row, output column).  align=False: the
    MUTATION `align_corners=False`, as in upsample_ref."""
    n, c, h, w = x.shape
    y0, y1, ly, hy = (t[oys] for t in up_axis(h, align=align))
    x0, x1, lx, hx = (t[oxs] for t in up_axis(w, align=align))
    g = lambda yy, xx: x[ns, :, yy, xx].double()
    return hy[:, None] * (hx[:, None] * g(y0, x0) + lx[:, None] * g(y0, x1)) + ly[:, None] * (hx[:, None] * g(y1, x0) + lx[:, None] * g(y1, x1))


def upsample_sample_points(n, h, w):
    """Seeded output positions of the sampled case: the corners and last pixels of every sample + UP_SAMPLES random ones."""
    rs = np.random.RandomState(seed_of(4, n, h, w))
    ns, oys, oxs = rs.randint(0, n, UP_SAMPLES), rs.randint(0, 2 * h, UP_SAMPLES), rs.randint(0, 2 * w, UP_SAMPLES)
    cy, cx = [0, 0, 2 * h - 1, 2 * h - 1, 2 * h - 1], [0, 2 * w - 1, 0, 2 * w - 1, 2 * w - 2]
    ns = np.concatenate([ns] + [[k] * 5 for k in range(n)])
    oys, oxs = np.concatenate([oys] + [cy] * n), np.concatenate([oxs] + [cx] * n)
    return torch.from_numpy(ns).long(), torch.from_numpy(oys).long(), torch.from_numpy(oxs).long()


# ---------------------------------------------------------------------------------------------------------------------
# decoders of a consumer tensor [n, c8_total, 2, h, w, 8] (f16), given the window (cg0, c_out)
# ---------------------------------------------------------------------------------------------------------------------

def outside_mask(t, cg0, co):
    """True for every 16-bit word of t that lies outside channel groups cg0 .. cg0 + c_out / 8 - 1."""
    m = torch.ones(t.shape, dtype=torch.bool)
    m[:, cg0:cg0 + (co + 7) // 8] = False
    return m


def _nchw(planes, co):
    n, c8, h, w, _ = planes.shape
    return planes.permute(0, 1, 4, 2, 3).reshape(n, c8 * 8, h, w)[:, :co]


def decode_h2(t, cg0, co):
    """(hi + lo as float64 [n, c_out, h, w], mask of the words outside the window)"""
    body = t[:, cg0:cg0 + (co + 7) // 8].double()
    return _nchw(body[:, :, 0] + body[:, :, 1], co), outside_mask(t, cg0, co)


def decode_f8(t, cg0, co):
    """(hi + fp8(xl 2^9) / 512, the 4 fp8(v / 4) plane, mask): the lo slot of a chunk's even group holds the 16 fp8(xl 2^9) bytes of
    the 16-channel chunk, the lo slot of its odd group the 16 fp8(v / 4) bytes (the byte layout of test_hip_up2v_runs._decode_f8)."""
    assert cg0 % 2 == 0 and co % 16 == 0
    body = t[:, cg0:cg0 + co // 8]
    n, c8, _, h, w, _ = body.shape
    hi = _nchw(body[:, :, 0].double(), co)
    lo = body[:, :, 1].contiguous().view(torch.uint8).view(torch.float8_e4m3fn).double()          # [n, c8, h, w, 16]
    xl = lo[:, 0::2].permute(0, 1, 4, 2, 3).reshape(n, c8 * 8, h, w)[:, :co]
    xh = lo[:, 1::2].permute(0, 1, 4, 2, 3).reshape(n, c8 * 8, h, w)[:, :co]
    return hi + xl / 512, xh * 4, outside_mask(t, cg0, co)


# ---------------------------------------------------------------------------------------------------------------------
# bounds
# ---------------------------------------------------------------------------------------------------------------------

def tol_f32(in_fmt, lin, osc=None, rel=None):
    """rel: a relative bound other than B_FMT[in_fmt] (the stem's STEM_B)."""
    s = 1.0 if osc is None else max(1.0, float(osc.abs().max()))
    return (B_FMT[in_fmt] if rel is None else rel) * float(lin.abs().max()) * s


def tol_decoded(in_fmt, out_fmt, lin, want, osc=None, rel=None):
    return tol_f32(in_fmt, lin, osc, rel) + KEEP_FMT[out_fmt] * float(want.abs().max())


def tol_plane(want):
    return FP8_PLANE * float(want.abs().max())


def tol_route(in_fmt, route, lin, want, osc):
    out_fmt = ROUTES[route][0]
    return tol_f32(in_fmt, lin, osc) if out_fmt is None else tol_decoded(in_fmt, out_fmt, lin, want, osc)


def tol_upsample(x, out_fmt, want):
    return UP_B * float(x.abs().max()) + KEEP_FMT[out_fmt] * float(want.abs().max())


# ---------------------------------------------------------------------------------------------------------------------
# what a case must hold, and the mutations it must catch
# ---------------------------------------------------------------------------------------------------------------------

def blocks_missing_a_sign(pre, th, tw, cs):
    """Blocks (sample, channel, row, column) -- one sample x cs channels x th rows x tw columns, clipped to the image -- whose
    pre-activations are all of one sign (empty = every workgroup's epilogue meets the kink)."""
    n, co, ho, wo = pre.shape
    bad = []
    for k in range(n):
        for c0 in range(0, co, cs):
            for y0 in range(0, ho, th):
                for x0 in range(0, wo, tw):
                    p = pre[k, c0:c0 + cs, y0:y0 + th, x0:x0 + tw]
                    if not (bool((p > 0).any()) and bool((p < 0).any())):
                        bad.append((k, c0, y0, x0))
    return bad


def conv_mutations(kind, stride, ci, co, ho, wo, scaled):
    """name -> mutated `want` of a conv case (scaled: with the output scales): what a subtly wrong kernel would compute."""
    d = conv_inputs(kind, stride, ci, co, ho, wo)
    x, w, b = d["x"], d["w"], d["b"]
    osc = oscale_of(d, co) if scaled else None
    lin = conv_lin(kind, stride, ci, co, ho, wo)
    out = {"replicate padding": finish(_lin(x, w, stride, "replicate"), b, SLOPE, osc)}
    if stride == 2:
        out["stride-2 window from 2i"] = finish(_lin(x, w, 2, even_window=True), b, SLOPE, osc)
    if scaled:
        out["oscale before the lrelu"] = lrelu((lin + b.double()[None, :, None, None]) * osc.double()[:, :, None, None])
        out["oscale rows read with stride c_out"] = finish(lin, b, SLOPE, oscale_of(d, co, row_stride=co))
    slice_co = CO_WG if kind == 0 else SMALL_CO
    if co > slice_co:
        out["later c_out slices with the first slice's bias"] = finish(lin, b[torch.arange(co) % slice_co], SLOPE, osc)
    k0 = (ci - 1) // 16 * 16                                   # first channel of the last 16-channel chunk
    out["last chunk dropped"] = finish(lin - _lin(x[:, k0:], w[:, k0:], stride), b, SLOPE, osc)
    if ci % 16:
        # the ragged chunk's padding channels hold the chunk's own first channels (activations and weights) instead of zeros
        k1 = k0 + 16 - ci
        out["ragged chunk's padding channels non-zero"] = finish(lin + _lin(x[:, k0:k0 + k1], w[:, k0:k0 + k1], stride), b, SLOPE, osc)
    return out


def stem_mutations(n, h, w, preproc):
    d = stem_inputs(n, h, w)
    out = {"replicate padding": lrelu(F.conv2d(F.pad(preprocess(d["x"], preproc), (3, 3, 3, 3), mode="replicate"), d["w"].double())
                                      + d["b"].double()[None, :, None, None]),
           "taps transposed": stem_ref(d["x"], d["w"], d["b"], preproc, transposed=True)[1]}
    if preproc:
        out["preprocessing 1 <-> 2"] = stem_ref(d["x"], d["w"], d["b"], 3 - preproc)[1]
    return out


def upsample_mutations(n, c, h, w):
    x = upsample_input(n, c, h, w)
    out = {"align_corners=False": upsample_ref(x, align=False)}
    if h != w:
        out["h and w swapped in the scale"] = upsample_ref(x, swap=True)
    return out
