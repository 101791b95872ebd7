"""float64 restatement of one modulated 3 x 3 layer with a LIVE epilogue -- demodulation, noise, bias, leaky ReLU, gain, clamp, the
consumer's styles, the fused ToRGB -- the seeded inputs that put every workgroup's epilogue on both sides of kink and clamp, the
case tables of tests/test_hip_conv_forms_f64.py (every form of the split-f16 up=1 kernel, the older up=2 tiles, the small-image
kernels) and of tests/test_hip_up2v_forms_f64.py (the 36 instantiations of the pipelined up=2 kernel, its tile loop, its in-kernel
noise, the launcher's selection: UP2V_*, up2v_*) and the mutated references that tests/test_conv_form_refs_cpu.py uses to show that
these cases can tell a wrong kernel from a right one.  TEST INFRASTRUCTURE: no GPU, no library call; plain torch in float64.

Reference (the method of tests/test_hip_up2v_runs.py):
    lin = conv(x * s, w) * dco              (_conv_ref of tests/test_hip_f8.py, up = 1 and up = 2)
    pre = (lin + noise + bias) * GAIN;  act = lrelu(pre);  ref = clamp(act);  want = ref * next style
and _torgb_ref of tests/test_hip_step_kernels.py applied to ref for the fused ToRGB.

Bounds, all from the project (tests/test_hip_f8.py, tests/test_hip_f6.py, tests/test_hip_up2v_runs.py):
    fp32 output   B x max|lin| x GAIN, B = 2e-6 (hi / lo f16 operands), 4e-5 ("f8"), 8e-5 ("f6"); noise, bias, lrelu and clamp
                  follow the linear output and are 1-Lipschitz, so the bound holds behind them
    hand-off      that bound x the largest next style + what the format keeps (2^-21 of the largest value for hi + lo f16, 2e-5
                  for hi + fp8 residual); the fp8(v / 4) plane within 0.07 of the largest value; operands of one format into the
                  container of another (up2v): the operands' B, the container's keep (tol_handoff_x)
    hi-only       (operand format 3) 5e-6 x max|lin| x GAIN against the float64 product of the f16-ROUNDED operands (linear_hi)
    ToRGB         _torgb_ref's own bounds with the conv bound carried into the logits: E += tol_conv x sum_c |w_c s_c|"""
import functools

import numpy as np
import torch

from test_hip_f8 import _conv_ref
from test_hip_step_kernels import _torgb_ref

ALPHA, GAIN, CLAMP = 0.2, 1.4142135, 3.0
# operand format (0 H2, 1 f8, 2 f6; 3 = f8 operands, hi halves only: against the float64 product of the f16-ROUNDED operands, the 5e-6 of
# test_hi_only_form_is_the_plain_f16_product) -> bound relative to max|lin| x GAIN
B_FMT = {0: 2e-6, 1: 4e-5, 2: 8e-5, 3: 5e-6}
FMT_NAME = {0: "h2", 1: "f8", 2: "f6", 3: "hi"}
KEEP_FMT = {0: 2.0 ** -21, 1: 2e-5}                  # what the hand-off format keeps of the largest value (H2, f8)
FP8_PLANE = 0.07                                     # fp8(v / 4) plane: one fp8 step
CATCH = 20                                           # a mutation must move the reference by this many bounds
SMALL_FLAT = 5e-5                                    # the flat tolerance the small-image kernels had until now (upper limit of SMALL_B)
# small-image kernels: 4 x the worst ratio |y - float64| / (max|lin| x GAIN) observed on an MI355X over every case of small_cases():
# 3.40e-7 (up = 1) and 6.06e-7 (up = 2, whose weights are FIR-folded in fp32 first); figures per case in the docstring of
# test_small_kernels_vs_float64 and in DESIGN.md 5
SMALL_B = 4 * 6.06e-7


# ---------------------------------------------------------------------------------------------------------------------
# case tables
# ---------------------------------------------------------------------------------------------------------------------

# up = 1 shapes: name -> (n, ci, co, h, w)
UP1_SHAPES = {
    "A": (3, 32, 48, 16, 32),     # MW = 1; ragged c_out inside the one slice; % 16 for the f8 / f6 hand-off; one full-height tile, two half-height
    "B": (2, 48, 96, 32, 64),     # MW = 2, 96 of 128; tile boundaries in both directions in every form
    "C": (5, 40, 136, 16, 32),    # H2 only: odd number of channel groups (zero-page group, round-3 loop whatever is asked for); 8 of 128 in slice 2
    "D": (2, 16, 64, 48, 32),     # one chunk: the K loop is prologue and tail only; three / six tile rows
    "E": (2, 32, 36, 16, 32),     # c_out % 8 != 0: fp32 and ToRGB-from-LDS only
    "P": (70, 16, 64, 32, 64),    # persistent forms, one workgroup per CU: 280 items on 256 workgroups, ragged shares, tile loop taken
}
# fused-ToRGB settings per shape: (render mode, ToRGB clamp, partly-NaN user colors, sfactor)
TORGB_SETTINGS = {"A": (1, 256.0, True, False), "B": (0, 0.5, False, True), "D": (0, -1.0, True, True), "E": (1, 0.5, False, False),
                  "P": (0, 256.0, False, False)}

# up = 1 forms: name -> dict(fmt, rows, v2, pp, persist, small); "small" = modconv3x3_up1_h3s_kernel (H2 only)
UP1_FORMS = {}
for _fmt in (0, 1):
    for _loop, _v2 in (("old", 0), ("pipe", 1)):
        for _rows in (1, 2):
            UP1_FORMS[f"{FMT_NAME[_fmt]}-{_loop}{_rows}"] = dict(fmt=_fmt, rows=_rows, v2=_v2, pp=0, persist=0, small=0)
UP1_FORMS["h2-pipe2-persist"] = dict(fmt=0, rows=2, v2=1, pp=0, persist=1, small=0)
UP1_FORMS["h2-h3s"] = dict(fmt=0, rows=2, v2=1, pp=0, persist=0, small=1)
UP1_FORMS["f8-pp2"] = dict(fmt=1, rows=2, v2=1, pp=1, persist=0, small=0)
UP1_FORMS["f8-pp2-persist"] = dict(fmt=1, rows=2, v2=1, pp=1, persist=1, small=0)
UP1_FORMS["f6-pipe1"] = dict(fmt=2, rows=1, v2=1, pp=0, persist=0, small=0)
UP1_FORMS["f6-pipe2"] = dict(fmt=2, rows=2, v2=1, pp=0, persist=0, small=0)
# the remaining full-height instantiations have a persistent twin as well (the launcher's NB_H3_GO): on B (MW = 2) and P (MW = 1) only
for _name in ("h2-old2", "f8-old2", "f8-pipe2", "f6-pipe2"):
    UP1_FORMS[_name + "-persist"] = dict(UP1_FORMS[_name], persist=1, shapes=("B", "P"))


def up1_tile(form, co):
    """(tile rows, c_out per workgroup) of an up = 1 form: 8 waves as MW x (8 / MW), `rows` pixel rows of 32 per wave; h3s: 8 x 64."""
    f = UP1_FORMS[form]
    if f["small"]:
        return 8, 64
    mw = 2 if co > 64 else 1
    return (8 // mw) * f["rows"], 64 * mw


def up1_routes(form, shape):
    """Output routes of an up = 1 (form, shape) as the launcher allows them."""
    f = UP1_FORMS[form]
    n, ci, co, h, w = UP1_SHAPES[shape]
    div = 8 if f["fmt"] == 0 else 16
    routes = ["f32"]
    if shape in ("A", "B"):
        routes += ["f32-shared", "f32-null"]              # shared noise (stride 0) and null noise with the bias live
    if co % div == 0:
        routes.append("handoff")                          # (the form's own format; c_next > c_out, next_stride > c_next)
    if shape in TORGB_SETTINGS and (not f["small"] or co <= 64):
        # MW = 1, no fp32 output, c_out % 8 == 0: from the accumulators; everything else from the LDS image (h3s: its own LDS image)
        routes.append("torgb")
        if shape == "A":
            routes.append("torgb-tap")                    # the fp32 output tapped as well: the LDS route on an MW = 1 kernel
    return routes


def up1_cases():
    """[(form, shape, route)]: every form on A, B, D and E; the H2 forms on C; the persistent forms on P (the four persistent
    twins beyond "pipelined H2" and "ping-pong f8" on B and P only)."""
    out = []
    for form, f in UP1_FORMS.items():
        shapes = ["A", "B", "D", "E"] + (["C"] if f["fmt"] == 0 else []) + (["P"] if f["persist"] else [])
        shapes = list(f.get("shapes", shapes))
        for s in shapes:
            if f["fmt"] and UP1_SHAPES[s][1] % 16:
                continue
            out += [(form, s, r) for r in up1_routes(form, s)]
    return out


# older up = 2 forms (modconv3x3_up2_h3_kernel): name -> (tile hook, pair hook, quad rows per tile, quad columns per tile)
UP2_FORMS = {"t12": (12, 0, 12, 32), "t8": (8, 0, 8, 32), "t5": (5, 0, 5, 32), "pair": (12, 1, 12, 16)}
# (ci, co, h, w, n): the five shapes of test_up2v_runs_vs_float64 ...
UP2_SHAPES = [(32, 32, 8, 32, 1), (32, 64, 14, 64, 3), (48, 32, 25, 32, 2), (32, 32, 26, 32, 2), (32, 96, 13, 64, 5)]
# ... the 16-wide form (8 x 16 tiles: ragged and several tile rows) and the 8-wide form (8 x 8 tiles; 16 x 8 = two tile rows, which
# the launcher accepts and nothing ran: the kernel's loads, noise reads and stores are guarded by the image's height exactly as
# in the 16-wide instantiation, see the test's docstring)
UP2_NARROW = [("w16", 32, 64, 8, 16, 3), ("w16", 32, 64, 12, 16, 3), ("w16", 32, 64, 24, 16, 2), ("w8", 32, 64, 8, 8, 3),
              ("w8", 32, 64, 16, 8, 3)]


def up2_cases():
    """[(form, fmt, ci, co, h, w, n, route)]"""
    out = []
    for form in UP2_FORMS:
        for fmt in ((0,) if form == "pair" else (0, 1)):          # (the two-workgroups-per-CU form takes H2 operands only)
            out += [(form, fmt) + s + (r,) for s in UP2_SHAPES for r in ("f32", "handoff")]
    for form, ci, co, h, w, n in UP2_NARROW:
        out += [(form, fmt, ci, co, h, w, n, r) for fmt in (0, 1) for r in ("f32", "handoff")]
    return out


def up2_tile(form):
    return {"w16": (8, 16), "w8": (8, 8)}.get(form) or UP2_FORMS[form][2:]


# the pipelined up = 2 kernel (modconv3x3_up2v_kernel, tests/test_hip_up2v_forms_f64.py): name -> (nb_debug_set_up2v_rows,
# nb_debug_set_up2v_persistent).  36 instantiations: 3 forms x operand format 0 .. 3 x output (fp32, H2 container, f8 container)
UP2V_FORMS = {"r12p": (12, 1), "r12": (12, 0), "r13": (13, -1)}
UP2V_FMTS = (0, 1, 2, 3)
UP2V_ROUTES = ("f32", "f32-shared", "f32-null", "handoff-h2", "handoff-f8")
UP2V_CUS = 256                    # compute units of an MI355X: the persistent grid of the tile-loop cases at one workgroup per CU
# name -> (n, ci, co, h, w)
UP2V_SHAPES = {
    "A": (2, 16, 48, 13, 32),     # one live chunk (prologue and tail only); ragged second slice; exactly one 13-row tile, 12 + 1 at 12 rows
    "B": (3, 64, 64, 14, 64),     # four chunks; two tile columns, two slices: 24 items, the XCD-renumbered order; last tile 1 or 2 rows
    "C": (2, 80, 96, 27, 32),     # five chunks; three slices in co_ld 128 (no fourth); three tile rows at both heights
    "D": (1, 112, 36, 8, 128),    # seven chunks; c_out % 8 != 0 (fp32 only); four tile columns; image shorter than a tile
    "N": (3, 32, 32, 32, 32),     # square output: the in-kernel noise case
    "P1": (35, 16, 64, 24, 64),   # 280 items on 256 workgroups: total and grid multiples of 8, the renumbered order; full tiles only
    "P2": (47, 32, 64, 25, 32),   # 282 items: the plain order; every third tile is one row high
    # launcher selection, every hook at its default.  S12 is NOT the (20, 16, 128, 24, 32) first proposed for it: nb_up2_h3_select takes
    # the 8-row tiles of the older kernel there (240 workgroups in one round at 3.93 against 160 at 5.4).  This is the smallest output
    # at c_in 16, c_out <= 128, w = 32 for which the selection is up2v with 12-row tiles (up2v_select below restates the launcher's
    # arithmetic; searched over n < 200, h < 80): 160 workgroups, the least that keeps the 12-row tiles, each tile 9 rows of 12
    "S12": (40, 16, 128, 9, 32),
    "S13": (28, 16, 128, 50, 32),
}


def up2v_select(ci, co, n, h, w, ncu=UP2V_CUS):
    """What nb_up2_h3_select and nb_up2v_rows answer for an f8 launch with every hook at its default, restated: (kernel, rows).
    The GPU test asks the library itself (nb_modconv3x3_up2_h3_variant, nb_debug_up2v_auto_rows) before it launches; this is how
    the shapes S12 / S13 were found, and test_conv_form_refs_cpu.py holds them to it."""
    tiles_x, slices, nch = w // 32, (co + 31) // 32, (ci + 15) // 16
    cdiv = lambda a, b: (a + b - 1) // b
    big, mid = n * tiles_x * cdiv(h, 12) * slices, n * tiles_x * cdiv(h, 8) * slices
    if big < 160 or cdiv(mid, 256) * 3.93 < 0.9 * cdiv(big, 256) * 5.4 or ci % 16 or w % 32 or h < 8:
        return "modconv3x3_up2_h3_kernel", 0

    def est(tqh, rest):
        ty = cdiv(h, tqh)
        s = sum(0.44 * nch * cdiv(cdiv((min(tqh, h - t * tqh) + 2) * 34, 32), 4) + rest for t in range(ty))
        return cdiv(n * tiles_x * ty * slices, ncu) * (s / ty)
    return "modconv3x3_up2v_kernel", 13 if est(13, 19.7) < 0.98 * est(12, 18.5) else 12


def up2v_routes(shape):
    """Output routes of a shape as the launcher allows them: shared / null noise on B and C; H2 output needs c_out % 8 == 0, f8
    output c_out % 16 == 0."""
    co = UP2V_SHAPES[shape][2]
    return [r for r in UP2V_ROUTES if (r == "f32" or (r in ("f32-shared", "f32-null") and shape in ("B", "C"))
                                       or (r == "handoff-h2" and co % 8 == 0) or (r == "handoff-f8" and co % 16 == 0))]


def up2v_cases():
    """[(form, fmt, shape, route)]: every form x operand format x route on A .. D."""
    return [(form, fmt, s, r) for form in UP2V_FORMS for fmt in UP2V_FMTS for s in "ABCD" for r in up2v_routes(s)]


def up2v_loop_cases():
    """[(form, fmt, shape, route)]: the tile loop -- both 12-row forms on P1 / P2 at one persistent workgroup per CU."""
    return [(form, fmt, s, r) for form in ("r12p", "r12") for fmt in (0, 1) for s in ("P1", "P2") for r in ("f32", "handoff-" + FMT_NAME[fmt])]


def up2v_noise_mode(route):
    return {"f32-shared": "shared", "f32-null": "null"}.get(route, "per")


def up2v_geometry(shape, rows):
    """(tiles_x, tiles_y, slices, items_x, items) of a launch, as nb_up2v_launch sets them."""
    n, ci, co, h, w = UP2V_SHAPES[shape]
    tiles_x, tiles_y, slices = w // 32, (h + rows - 1) // rows, (co + 31) // 32
    return tiles_x, tiles_y, slices, tiles_x * tiles_y * slices, tiles_x * tiles_y * slices * n


def up2v_item(l, items, items_x, slices, tiles_x, grid):
    """Item l of a launch of `grid` workgroups -> (sample, tile_y, tile_x, slice): tile_coords of modconv3x3_up2v_kernel restated
    (no order flags).  The whole list is renumbered into eighths when list and grid are multiples of 8, else a sample's items are
    where its own count is."""
    nn, b = divmod(l, items_x)
    if items % 8 == 0 and grid % 8 == 0:
        nn, b = divmod((l & 7) * (items >> 3) + (l >> 3), items_x)
    elif items_x % 8 == 0:
        b = (((b & 7) + nn) & 7) * (items_x >> 3) + (b >> 3)
    b, sl = divmod(b, slices)
    ty, tx = divmod(b, tiles_x)
    return nn, ty, tx, sl


# small-image kernels: (up, n, c1, c2, co, h, waves, blocks, noise); blocks = 2 only where the launcher's can_two holds (eight waves,
# one sample per tile, an even number of tile rows)
def small_cases():
    out = []
    for up in (1, 2):
        c2s = (0,) if up == 1 else (0, 16)                        # (the concatenated second input exists for up = 2)
        for n, h in ((3, 4), (2, 8), (2, 16), (2, 64)):
            for c2 in c2s:
                for waves in (4, 8):
                    out.append((up, n, 32, c2, 40, h, waves, 1, "per"))
                if h >= 8:
                    out.append((up, n, 32, c2, 40, h, 8, 2, "per"))
            out += [(up, n, 32, 0, 40, h, 4, 1, "shared"), (up, n, 32, 0, 40, h, 8, 1, "null")]
    return out


def small_tile(up, h):
    """(output rows, output columns, samples) of one workgroup's 32 positions (one block per tile)."""
    if h >= 32:
        return up, 32 * up, 1
    if h * h >= 32:
        return (32 // h) * up, h * up, 1
    return h * up, h * up, 2


# ---------------------------------------------------------------------------------------------------------------------
# inputs and reference
# ---------------------------------------------------------------------------------------------------------------------

# cases whose first seed leaves a workgroup's block short of kink or clamp (tests/test_conv_form_refs_cpu.py says which): the next
# seed that does not
SEED_SALT = {(1, 3, 32, 40, 4, 4): 1, (2, 48, 14, 18, 4, 32): 1}


def seed_of(up, n, ci, co, h, w):
    return (up * 100003 + n * 7919 + ci * 131 + co * 17 + h * 5 + w + 1000003 * SEED_SALT.get((up, n, ci, co, h, w), 0)) % (2 ** 31)


def c_next_of(co):
    """Consumer channels of the hand-off cases: more than the producer writes (whole 16-channel chunks)."""
    return (co + 15) // 16 * 16 + 16


@functools.lru_cache(maxsize=None)
def inputs(up, n, ci, co, h, w):
    """Seeded fp32 inputs of one layer (CPU tensors).  noise is [n, up h, up w]: shared-noise cases use sample 0 for everyone."""
    rs = np.random.RandomState(seed_of(up, n, ci, co, h, w))
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    c_next = c_next_of(co)
    d = dict(x=f(rs.randn(n, ci, h, w)), w=f(rs.randn(co, ci, 3, 3) / np.sqrt(9 * ci)), st=f(rs.uniform(0.5, 1.5, (n, ci))),
             dco=f(rs.uniform(0.5, 1.5, (n, co))), bias=f(1.5 * rs.randn(co)), noise=f(rs.randn(n, up * h, up * w)),
             nst=f(rs.uniform(0.5, 1.5, (n, c_next + 8))))                       # (row stride c_next + 8 > c_next)
    # fused ToRGB operands: styles rows = 9 color scalars + c_out styles + 3 spare; user colors half NaN; sfactor below 1, above 1, s' = 1
    tst = rs.uniform(0.5, 1.5, (n, co + 12))
    tst[:, :9] = 1.5 * rs.randn(n, 9)
    uc = rs.rand(n, 9)
    uc[rs.rand(n, 9) < 0.5] = np.nan
    sf = np.array([0.5, 1.7, 1e9] + [float(rs.choice([0.3, 1.5, 3.0])) for _ in range(max(n - 3, 0))])[:n]
    d.update(tst=f(tst), tw=f(rs.randn(3, co) / np.sqrt(co)), tb=f(rs.randn(3)), cb=f(rs.randn(9)), uc=f(uc), sf=f(sf))
    return d


@functools.lru_cache(maxsize=None)
def linear(up, n, ci, co, h, w):
    """lin = conv(x * s, w) * dco in float64: computed once per shape, shared by every test of that shape, never written to."""
    d = inputs(up, n, ci, co, h, w)
    return _conv_ref(d["x"], d["w"], d["st"], up) * d["dco"].double()[:, :, None, None]


@functools.lru_cache(maxsize=None)
def linear_hi(up, n, ci, co, h, w):
    """lin of the hi-only operand format (3): the float64 convolution of the f16-ROUNDED operands, (x * st).half() and w.half(), as in
    test_hi_only_form_is_the_plain_f16_product -- what a plain single-f16 evaluation with exact accumulation gives."""
    d = inputs(up, n, ci, co, h, w)
    xr = (d["x"] * d["st"][:, :, None, None]).half().float()
    return _conv_ref(xr, d["w"].half().float(), torch.ones_like(d["st"]), up) * d["dco"].double()[:, :, None, None]


def noise_of(d, noise):
    """float64 [n or 1, 1, H, W] noise image of a noise mode ("per", "shared" = sample 0 for everyone, "null"), or of a noise
    tensor [n, H, W] given in its place (the in-kernel noise case)."""
    if torch.is_tensor(noise):
        return noise.double()[:, None]
    nz = d["noise"].double()[:, None]
    return nz if noise == "per" else nz[:1] if noise == "shared" else torch.zeros_like(nz[:1])


def epilogue(lin, d, noise="per", clamp=CLAMP, clamp_first=False):
    """(pre, act, ref) of the live epilogue behind lin.  clamp_first: the MUTATION `clamp before the gain`."""
    t = lin + noise_of(d, noise) + d["bias"].double()[None, :, None, None]
    if clamp_first:
        a = torch.where(t >= 0, t, ALPHA * t)
        return t * GAIN, a * GAIN, a.clamp(-clamp, clamp) * GAIN
    pre = t * GAIN
    act = torch.where(pre >= 0, pre, ALPHA * pre)
    return pre, act, act.clamp(-clamp, clamp)


def reference(up, n, ci, co, h, w, noise="per", hi=False):
    """dict(lin, pre, act, ref, scale = max|lin| x GAIN) of a case.  hi: the hi-only operand format's reference (linear_hi)."""
    d = inputs(up, n, ci, co, h, w)
    lin = (linear_hi if hi else linear)(up, n, ci, co, h, w)
    pre, act, ref = epilogue(lin, d, noise)
    return dict(lin=lin, pre=pre, act=act, ref=ref, scale=float(lin.abs().max()) * GAIN)


def tol_f32(fmt, scale, b=None):
    return (B_FMT[fmt] if b is None else b) * scale


def handoff_want(d, ref, co):
    return ref * d["nst"].double()[:, :co, None, None]


def tol_handoff(fmt, scale, d, want, co):
    """Bound of the decoded hand-off operand (H2: hi + lo; f8: hi + fp8 residual / 512)."""
    return tol_f32(fmt, scale) * float(d["nst"][:, :co].max()) + KEEP_FMT[min(fmt, 1)] * float(want.abs().max())


def tol_handoff_x(fmt, out_fmt, scale, d, want, co):
    """Bound of a decoded hand-off operand whose container (out_fmt: 0 H2, 1 f8) need not be the operands' format (fmt 0 .. 3):
    B_FMT[fmt] x scale x the largest next style + what the container keeps of the largest value.  fmt == out_fmt: tol_handoff."""
    return tol_f32(fmt, scale) * float(d["nst"][:, :co].max()) + KEEP_FMT[out_fmt] * float(want.abs().max())


def torgb_reference(d, ref, co, shape, tol_conv):
    """_torgb_ref on the float64 conv output with the conv's bound carried into the logits -> (dict name -> (want, tol), ambiguous)."""
    mode, clamp, ucol, sfk = TORGB_SETTINGS[shape]
    n = ref.shape[0]
    return _torgb_ref(ref.reshape(n, co, -1), d["tst"], d["tw"], d["tb"], d["cb"], clamp, d["uc"] if ucol else None,
                      d["sf"] if sfk else None, mode, co, x_err=tol_conv)


# ---------------------------------------------------------------------------------------------------------------------
# what a case must hold, and the mutations it must catch
# ---------------------------------------------------------------------------------------------------------------------

def blocks_meet_kink_and_clamp(pre, act, th, tw, cs, spt=1):
    """Every workgroup's block of outputs -- `spt` samples x cs channels x th rows x tw columns -- has pre-activations of both
    signs and |act| on both sides of CLAMP.  Returns the list of blocks that do not (empty = fine)."""
    n, co, ho, wo = pre.shape
    bad = []
    for n0 in range(0, n, spt):
        for c0 in range(0, co, cs):
            for y0 in range(0, ho, th):
                for x0 in range(0, wo, tw):
                    p = pre[n0:n0 + spt, c0:c0 + cs, y0:y0 + th, x0:x0 + tw]
                    a = act[n0:n0 + spt, c0:c0 + cs, y0:y0 + th, x0:x0 + tw].abs()
                    if not (bool((p > 0).any()) and bool((p < 0).any()) and bool((a > CLAMP).any()) and bool((a < CLAMP).any())):
                        bad.append((n0, c0, y0, x0))
    return bad


def mutations(up, n, ci, co, h, w, noise, th):
    """name -> mutated `ref` of a case: what a subtly wrong kernel would compute.  th = output rows per tile of the form."""
    d = inputs(up, n, ci, co, h, w)
    lin = linear(up, n, ci, co, h, w)
    ref = epilogue(lin, d, noise)[2]
    out = {}
    # one input channel zeroed: lin is linear in x, so the channel's own contribution is subtracted
    k = ci // 2
    part = _conv_ref(d["x"][:, k:k + 1], d["w"][:, k:k + 1], d["st"][:, k:k + 1], up) * d["dco"].double()[:, :, None, None]
    out["input channel zeroed"] = epilogue(lin - part, d, noise)[2]
    # the output shifted by one pixel row inside the first tile (one-row tiles: over the first two, i.e. a wrong tile row)
    m = ref.clone()
    rows = min(max(th, 2), ref.shape[2])
    m[:, :, :rows] = torch.roll(ref[:, :, :rows], 1, dims=2)
    out["row shifted inside a tile"] = m
    out["clamp omitted"] = epilogue(lin, d, noise)[1]
    out["clamp before the gain"] = epilogue(lin, d, noise, clamp_first=True)[2]
    if noise == "per" and n > 1:
        out["sample 0's noise for every sample"] = epilogue(lin, d, "shared")[2]
    elif noise == "shared" and n > 1:
        out["per-sample noise where it is shared"] = epilogue(lin, d, "per")[2]
    m = ref.clone()
    m[:, co - (co % 8 or 8):] = 0
    out["last c_out group zeroed"] = m
    return out


def up2v_second_items(shape, rows=12, grid=UP2V_CUS):
    """[(first item, later item)] as (sample, tile_y, tile_x, slice) for every item past a persistent workgroup's first one."""
    tiles_x, tiles_y, slices, items_x, items = up2v_geometry(shape, rows)
    it = lambda l: up2v_item(l, items, items_x, slices, tiles_x, min(grid, items))
    return [(it(l % grid), it(l)) for l in range(grid, items)]


def up2v_loop_mutations(shape, rows=12, grid=UP2V_CUS):
    """name -> (mutated ref, mutated hand-off value) of a tile-loop shape: what the persistent kernel would store if a workgroup
    carried per-tile state of its FIRST item into a later one -- the channel tables (load_channel_tables: dcoef x gain, bias x gain,
    next style) or the noise tile (write_noise; rows of the first tile below the image hold zero)."""
    UP = n, ci, co, h, w = UP2V_SHAPES[shape]
    d = inputs(2, *UP)
    lin, ref = linear(2, *UP), reference(2, *UP)["ref"]
    want = handoff_want(d, ref, co)
    dco, bias, nst, nz = d["dco"].double(), d["bias"].double(), d["nst"].double(), d["noise"].double()
    tiles_y = up2v_geometry(shape, rows)[1]
    nzp = torch.zeros(n, 2 * rows * tiles_y, 2 * w, dtype=torch.float64)
    nzp[:, :2 * h] = nz
    th = 2 * rows
    m_tab, w_tab, m_nz = ref.clone(), want.clone(), ref.clone()
    for (n1, y1, x1, s1), (n2, y2, x2, s2) in up2v_second_items(shape, rows, grid):
        c1, c2 = slice(32 * s1, min(32 * s1 + 32, co)), slice(32 * s2, min(32 * s2 + 32, co))
        ys, xs = slice(th * y2, min(th * y2 + th, 2 * h)), slice(64 * x2, 64 * x2 + 64)
        nrow = ys.stop - ys.start
        blk = lin[n2, c2, ys, xs]
        nz2 = nz[n2, ys, xs][None]
        # channel tables of the first item: its sample's dcoefs and next styles, its slice's biases
        t = blk / dco[n2, c2, None, None] * dco[n1, c1, None, None] + nz2 + bias[c1, None, None]
        p = t * GAIN
        a = torch.where(p >= 0, p, ALPHA * p).clamp(-CLAMP, CLAMP)
        m_tab[n2, c2, ys, xs] = a
        w_tab[n2, c2, ys, xs] = a * nst[n1, c1, None, None]
        # noise tile of the first item
        t = blk + nzp[n1, th * y1:th * y1 + nrow, 64 * x1:64 * x1 + 64][None] + bias[c2, None, None]
        p = t * GAIN
        m_nz[n2, c2, ys, xs] = torch.where(p >= 0, p, ALPHA * p).clamp(-CLAMP, CLAMP)
    return {"a workgroup's second item rendered with its first item's channel tables (dcoef, bias, next style)": (m_tab, w_tab),
            "a workgroup's second item rendered with its first item's noise tile": (m_nz, handoff_want(d, m_nz, co))}


# the in-kernel noise case (shape N, 64 x 64 output): a random constant, a non-zero strength, integer positions that are negative,
# beyond R and far beyond it; R = the image resolution of (positions % R) / (R - 1)
UP2V_NOISE_R = 256


@functools.lru_cache(maxsize=None)
def up2v_noise_case():
    """dict(nc [64, 64], lin [64], strength [1], pos int64 [n, 2], npos float32 [n, 2]) of shape N (CPU tensors)."""
    n, res = UP2V_SHAPES["N"][0], 2 * UP2V_SHAPES["N"][3]
    rs = np.random.RandomState(20250)
    nc = torch.from_numpy(rs.randn(res, res).astype(np.float32))
    pos = torch.tensor([[-3, 255], [UP2V_NOISE_R + 17, -300], [2 ** 40 + 5, -2 ** 40 - 77]], dtype=torch.int64)[:n]
    npos = torch.remainder(pos, UP2V_NOISE_R).to(torch.float32) / torch.tensor(UP2V_NOISE_R - 1, dtype=torch.float32)
    return dict(nc=nc, lin=torch.linspace(0, 1, res, dtype=torch.float32), strength=torch.tensor([1.25], dtype=torch.float32), pos=pos,
                npos=npos)


def up2v_noise_ref():
    """float64 [n, 64, 64] noise of up2v_noise_case by the oracle (shifted_const_noise: float32 sample coordinates, float64 blend), as
    test_noise_vs_float64 holds nb_noise_f32 to it."""
    from oracle import neube_oracle as orc
    c = up2v_noise_case()
    r = c["nc"].shape[0]
    grid = torch.stack([c["lin"][:, None].expand(r, r), c["lin"][None, :].expand(r, r)], dim=-1)
    return orc.shifted_const_noise(c["nc"].double(), grid, c["npos"])[:, 0] * float(c["strength"][0])
