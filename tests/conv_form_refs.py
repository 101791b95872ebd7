"""float64 restatement of one modulated 3 x 3 layer with a LIVE epilogue -- demodulation, noise, bias, leaky ReLU, gain, clamp, the
consumer's styles, the fused ToRGB -- the seeded inputs that put every workgroup's epilogue on both sides of kink and clamp, the
case tables of tests/test_hip_conv_forms_f64.py (every form of the split-f16 up=1 kernel, the older up=2 tiles, the small-image
kernels) and the mutated references that tests/test_conv_form_refs_cpu.py uses to show that these cases can tell a wrong kernel
from a right one.  TEST INFRASTRUCTURE: no GPU, no library call; plain torch in float64.

Reference (the method of tests/test_hip_up2v_runs.py):
    lin = conv(x * s, w) * dco              (_conv_ref of tests/test_hip_f8.py, up = 1 and up = 2)
    pre = (lin + noise + bias) * GAIN;  act = lrelu(pre);  ref = clamp(act);  want = ref * next style
and _torgb_ref of tests/test_hip_step_kernels.py applied to ref for the fused ToRGB.

Bounds, all from the project (tests/test_hip_f8.py, tests/test_hip_f6.py, tests/test_hip_up2v_runs.py):
    fp32 output   B x max|lin| x GAIN, B = 2e-6 (hi / lo f16 operands), 4e-5 ("f8"), 8e-5 ("f6"); noise, bias, lrelu and clamp
                  follow the linear output and are 1-Lipschitz, so the bound holds behind them
    hand-off      that bound x the largest next style + what the format keeps (2^-21 of the largest value for hi + lo f16, 2e-5
                  for hi + fp8 residual); the fp8(v / 4) plane within 0.07 of the largest value
    ToRGB         _torgb_ref's own bounds with the conv bound carried into the logits: E += tol_conv x sum_c |w_c s_c|"""
import functools

import numpy as np
import torch

from test_hip_f8 import _conv_ref
from test_hip_step_kernels import _torgb_ref

ALPHA, GAIN, CLAMP = 0.2, 1.4142135, 3.0
B_FMT = {0: 2e-6, 1: 4e-5, 2: 8e-5}                  # operand format (0 H2, 1 f8, 2 f6) -> bound relative to max|lin| x GAIN
FMT_NAME = {0: "h2", 1: "f8", 2: "f6"}
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
SEED_SALT = {(1, 3, 32, 40, 4, 4): 1}


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


def noise_of(d, noise):
    """float64 [n or 1, 1, H, W] noise image of a noise mode ("per", "shared" = sample 0 for everyone, "null")."""
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


def reference(up, n, ci, co, h, w, noise="per"):
    """dict(lin, pre, act, ref, scale = max|lin| x GAIN) of a case."""
    d = inputs(up, n, ci, co, h, w)
    lin = linear(up, n, ci, co, h, w)
    pre, act, ref = epilogue(lin, d, noise)
    return dict(lin=lin, pre=pre, act=act, ref=ref, scale=float(lin.abs().max()) * GAIN)


def tol_f32(fmt, scale, b=None):
    return (B_FMT[fmt] if b is None else b) * scale


def handoff_want(d, ref, co):
    return ref * d["nst"].double()[:, :co, None, None]


def tol_handoff(fmt, scale, d, want, co):
    """Bound of the decoded hand-off operand (H2: hi + lo; f8: hi + fp8 residual / 512)."""
    return tol_f32(fmt, scale) * float(d["nst"][:, :co].max()) + KEEP_FMT[min(fmt, 1)] * float(want.abs().max())


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
