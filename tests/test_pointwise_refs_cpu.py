"""CPU pin of tests/pointwise_refs.py: the float64 restatements of bias_act (three modes) and upfirdn2d (gather) reproduce the
reference-generated vectors of tests/golden/ops_kat.npz and tests/golden/ops_grads.npz at the tolerances the GPU tests use for
the same vectors; the input builders leave no element inside an excluded neighbourhood; and the ulp allowances K_ULPS that
tests/test_hip_pointwise_f64.py grants the device's math functions are 4x what the fp32 host oracle needs (at least 4)."""
import ast
import math

import numpy as np
import pytest
import torch

import pointwise_refs as pr
from conftest import load_golden
from oracle import neube_oracle as orc

T = torch.from_numpy


@pytest.fixture(scope="module")
def kg():
    return load_golden("ops_grads.npz")


@pytest.fixture(scope="module")
def kk():
    return load_golden("ops_kat.npz")


def close(got, want, tol):
    got = got.detach().numpy() if torch.is_tensor(got) else got
    assert got.shape == want.shape, (got.shape, want.shape)
    err = float(np.abs(got.astype(np.float64) - np.asarray(want, np.float64)).max())
    assert err <= tol, f"max abs err {err} > {tol}"


def _modes(x, b, dy, ddx, step_b, act, alpha, gain, clamp):
    """The six results of the autograd wrapper from the three modes of the restatement, as ops._BiasAct / _BiasActGrad chain
    them: yref is the forward rounded to fp32."""
    cfg = dict(act=act, alpha=alpha, gain=gain, clamp=clamp, step_b=step_b)
    y = pr.bias_act_ref(x, b, None, None, None, 0, **cfg)
    yref = y.float()
    dx = pr.bias_act_ref(dy, b, x, yref, None, 1, **cfg)
    d_dy = pr.bias_act_ref(ddx, b, x, yref, None, 1, **cfg)
    d_x = pr.bias_act_ref(ddx, b, x, yref, dy, 2, **cfg)
    return y, dx, d_dy, d_x


@pytest.mark.parametrize("act", pr.ACTS)
@pytest.mark.parametrize("tag,clamp", [("n", None), ("c", 0.8)])
def test_bias_act_ref_vs_golden_grads(kg, act, tag, clamp):
    x, b, dy, ddx = T(kg["ba_x"]), T(kg["ba_b"]), T(kg["ba_dy"]), T(kg["ba_ddx"])
    alpha, gain = pr.ACT_DEFAULTS[act]
    y, dx, d_dy, d_x = _modes(x, b, dy, ddx, 6 * 7, act, alpha, gain, -1 if clamp is None else clamp)
    p = f"ba_{act}_{tag}"
    close(y, kg[p + "_y"], 2e-6)
    close(dx, kg[p + "_dx"], 4e-6)
    close(dx.sum([0, 2, 3]), kg[p + "_db"], 4e-5)
    close(d_dy, kg[p + "_ddy"], 4e-6)
    close(d_x, kg[p + "_d2x"], 4e-6)
    close(d_x.sum([0, 2, 3]), kg[p + "_d2b"], 4e-5)
    # the same six through torch.autograd on the grad-0 restatement (what the wrapper test differentiates)
    xd, bd, dyd = (t.double().requires_grad_(True) for t in (x, b, dy))
    ya = pr.bias_act_ref(xd, bd, None, None, None, 0, act, alpha, gain, -1 if clamp is None else clamp, step_b=42)
    dxa, dba = torch.autograd.grad(ya, [xd, bd], dyd, create_graph=True)
    g2 = torch.autograd.grad((dxa * ddx.double()).sum(), [dyd, xd, bd], allow_unused=True)
    z = lambda t, like: torch.zeros_like(like) if t is None else t
    close(dxa, kg[p + "_dx"], 4e-6)
    close(dba, kg[p + "_db"], 4e-5)
    close(z(g2[0], dyd), kg[p + "_ddy"], 4e-6)
    close(z(g2[1], xd), kg[p + "_d2x"], 4e-6)
    close(z(g2[2], bd), kg[p + "_d2b"], 4e-5)


def test_bias_act_ref_vs_kats(kg, kk):
    x, b = T(kk["ba_x"]), T(kk["ba_b"])
    for act in ("lrelu", "linear", "tanh"):
        alpha, gain = pr.ACT_DEFAULTS[act]
        close(pr.bias_act_ref(x, b, None, None, None, 0, act, alpha, gain, -1, step_b=42), kk[f"ba_{act}_n"], 1e-6)
        close(pr.bias_act_ref(x, b, None, None, None, 0, act, alpha, gain, 1.5, step_b=42), kk[f"ba_{act}_c"], 1e-6)
    close(pr.bias_act_ref(x, b, None, None, None, 0, "lrelu", 0.2, np.sqrt(2) * 0.5, 128.0, step_b=42), kk["ba_lrelu_gain"], 1e-6)
    close(pr.bias_act_ref(T(kk["ba2_x"]), T(kk["ba2_b"]), None, None, None, 0, "tanh", 0, 1, -1, step_b=1), kk["ba2_tanh"], 1e-6)
    # bias along the last dimension with gain and alpha of its own, and its first-order gradient
    x, b, dy = T(kg["ba2_x"]), T(kg["ba2_b"]), T(kg["ba2_dy"])
    y = pr.bias_act_ref(x, b, None, None, None, 0, "lrelu", 0.1, 0.7, -1, step_b=1)
    dx = pr.bias_act_ref(dy, b, x, y.float(), None, 1, "lrelu", 0.1, 0.7, -1, step_b=1)
    close(y, kg["ba2_y"], 2e-6); close(dx, kg["ba2_dx"], 2e-6); close(dx.sum(0), kg["ba2_db"], 2e-5)


def _up(x, f, up=1, down=1, padding=(0, 0, 0, 0), flip_filter=False, gain=1.0):
    """The call surface of upfirdn2d.upfirdn2d on the gather: 1-D taps are a row pass then a column pass, sqrt(gain) each."""
    up = (up, up) if isinstance(up, int) else tuple(up)
    down = (down, down) if isinstance(down, int) else tuple(down)
    px0, px1, py0, py1 = padding
    if f.ndim == 2:
        return pr.upfirdn2d_ref(x, f, up, down, padding, flip_filter, gain)
    y = pr.upfirdn2d_ref(x, f[None, :], (up[0], 1), (down[0], 1), (px0, px1, 0, 0), flip_filter, math.sqrt(gain))
    return pr.upfirdn2d_ref(y, f[:, None], (1, up[1]), (1, down[1]), (0, 0, py0, py1), flip_filter, math.sqrt(gain))


def test_upfirdn2d_ref_vs_kats(kk):
    f, x = T(kk["fir_f"]), T(kk["fir_x"])
    close(_up(x, f, padding=[1, 1, 1, 1], gain=4), kk["fir_pad1_gain4"], 1e-6)
    close(_up(x, f, up=2, padding=[2, 1, 2, 1], gain=4), kk["fir_up2"], 1e-6)
    close(_up(x, f, down=2, padding=[1, 1, 1, 1]), kk["fir_down2"], 1e-6)
    close(_up(x, T(kk["fir_f_ragged"]), padding=[1, 0, 2, -1], flip_filter=True, gain=1.5), kk["fir_ragged_flip"], 1e-6)


@pytest.mark.parametrize("name", list("abcdeg"))
def test_upfirdn2d_ref_vs_golden_grads(kg, name):
    c = ast.literal_eval(str(kg[f"up_{name}_cfg"][0]))
    x = T(kg["up_x"]).double().requires_grad_(True)
    y = _up(x, T(kg["up_" + c["f"]]), up=c["up"], down=c["down"], padding=c["padding"], flip_filter=c["flip_filter"], gain=c["gain"])
    dx, = torch.autograd.grad(y, [x], T(kg[f"up_{name}_dy"]).double())
    close(y, kg[f"up_{name}_y"], 4e-6)
    close(dx, kg[f"up_{name}_dx"], 4e-6)


def test_upfirdn2d_ref_bound_counts_taps():
    """T of the bound: a 4x4 filter at up = 2 meets 2x2 samples inside the image, fewer at the border, none in a wide border."""
    x = torch.ones(1, 5, 5)
    y, tol = pr.upfirdn2d_ref(x, torch.ones(4, 4), (2, 2), (1, 1), (6, 6, 6, 6), False, 1.0, bound=True)
    assert y.shape == (1, 19, 19)
    assert float(y[0, 9, 9]) == 4 and float(tol[0, 9, 9]) == (4 + 2) * pr.U * 4
    assert float(y[0, 0, 0]) == 0 and float(tol[0, 0, 0]) == 0
    assert float(y[0, 3, 9]) == 2 and float(tol[0, 3, 9]) == (2 + 2) * pr.U * 2


@pytest.mark.parametrize("act", pr.ACTS)
def test_builders_leave_no_element_at_a_decision(act):
    """Every input set the GPU file builds (the builder runs with the clamp on; the set without a clamp has fewer conditions)."""
    alpha = pr.ACT_DEFAULTS[act][0]
    shapes = [((n,), None) for n in pr.SMALL_SIZES] + [(pr.BIAS_SHAPE, d) for d in (0, 1, 2)] + [(pr.ALIGN_SHAPE, 1)]
    if act in pr.WRAP_ACTS:
        shapes += [(s, 1) for s in pr.WRAP_SHAPES]
    for shape, dim in shapes:
        x, b, dy, ddx, step_b = pr.bias_act_inputs(shape, dim, act, alpha, pr.GAIN, pr.CLAMP, seed=pr.seed_of(shape, dim, act))
        assert x.dtype == np.float32 and x.shape == tuple(shape)
        for clamp in (pr.CLAMP, None):
            assert pr.count_offenders(x, b, step_b, act, alpha, pr.GAIN, clamp) == 0, (act, shape, dim, clamp)
        assert float(np.abs(x).max()) + (0 if b is None else float(np.abs(b).max())) < 70


def host_ulps(act, n=20000):
    """Largest error of the fp32 host oracle (oracle.neube_oracle.bias_act on float32 tensors, torch.autograd for the gradient
    modes) against the restatement on the same inputs, in ulps of the result and in excess of the restatement's own
    conditioning / rounding terms (K = 0), per mode; both clamp settings.  The gradient modes run without a bias and on
    |x| < 12 and get the unrounded forward as yref: autograd differentiates at x, not at a rounded x + b or a saved fp32 y."""
    alpha = pr.ACT_DEFAULTS[act][0]
    shape = (4, 8, n // 32)
    x0, b0, dy0, ddx0, step_b = pr.bias_act_inputs(shape, 1, act, alpha, pr.GAIN, pr.CLAMP, seed=pr.seed_of(shape, 1, act))
    x1 = pr.bias_act_inputs(shape, None, act, alpha, pr.GAIN, pr.CLAMP, seed=5)[0]               # (clear of the kinks without a bias)
    x1 = np.where(np.abs(x1) < 12, x1, np.float32(1.5))
    worst = [0.0, 0.0, 0.0]
    for clamp in (None, pr.CLAMP):
        cfg = dict(act=act, alpha=alpha, gain=pr.GAIN, clamp=-1 if clamp is None else clamp, step_b=step_b)
        y = orc.bias_act(T(x0), T(b0), dim=1, act=act, alpha=alpha, gain=pr.GAIN, clamp=clamp)
        x, dy = (T(a).clone().requires_grad_(True) for a in (x1, dy0))
        dx, = torch.autograd.grad(orc.bias_act(x, None, act=act, alpha=alpha, gain=pr.GAIN, clamp=clamp), [x], dy, create_graph=True)
        d_x, = torch.autograd.grad((dx * T(ddx0)).sum(), [x], allow_unused=True)
        d_x = torch.zeros_like(x) if d_x is None else d_x
        yref = pr.bias_act_ref(T(x1), None, None, None, None, 0, **cfg)
        refs = [pr.bias_act_ref(T(x0), T(b0), None, None, None, 0, K=0, **cfg),
                pr.bias_act_ref(T(dy0), None, T(x1), yref, None, 1, K=0, **cfg),
                pr.bias_act_ref(T(ddx0), None, T(x1), yref, T(dy0), 2, K=0, **cfg)]
        for m, (got, (want, tol0)) in enumerate(zip((y, dx, d_x), refs)):
            excess = ((got.detach().double() - want).abs() - tol0).clamp_min(0) / pr.ulp(want)
            worst[m] = max(worst[m], float(excess.max()))
    return worst


# gradient modes whose kernel expression calls no math function (they are arithmetic on yref), and the three that call expf
ARITHMETIC_GRADS = ("linear", "relu", "lrelu", "tanh", "elu", "selu")


NO_MATH = ("linear", "relu", "lrelu")


@pytest.mark.parametrize("act", pr.ACTS)
def test_k_ulps_are_four_times_the_host_oracle(act):
    """K_ULPS against the measurement m of this host: 0 for linear, relu and lrelu in every mode (no math function is called,
    m must be 0); otherwise at least 4 and 4 m <= K <= max(4, ceil(8 m)) -- an interval, since m depends on the host's libm
    (the figures in the docstring of tests/test_hip_pointwise_f64.py are one x86-64 host's).  For the gradient modes of sigmoid,
    softplus and swish the host figure (printed) is the conditioning of autograd's own formula on its rounded forward --
    hundreds to thousands of ulps, without limit as |x| grows -- and not the error of a math function; the kernel's only math
    call there is the expf that the forward measures, so those modes take the forward's K and this test requires just that."""
    got = host_ulps(act)
    print(f"host oracle ulps {act}: " + " ".join(f"grad{m} {v:.2f}" for m, v in enumerate(got)))
    K = pr.K_ULPS[act]
    if act in NO_MATH:
        assert K == (0, 0, 0) and got == [0.0, 0.0, 0.0]
        return
    for m in (0, 1, 2):
        if m == 0 or act in ARITHMETIC_GRADS:
            assert K[m] >= 4 and 4 * got[m] <= K[m] <= max(4, math.ceil(8 * got[m])), (m, got[m], K[m])
        else:
            assert K[m] == K[0]
