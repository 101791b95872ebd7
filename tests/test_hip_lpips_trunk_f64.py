"""GPU: the LPIPS trunk's convolutions, layer by layer, on every route ops.conv2d / ops._conv2d_input_grad take at painting size --
the split-f16 up = 1 kernel with the device ``tf`` weight pack in the backward, its embedded-canvas form for images that are no power
of two, the tiled fp32-MFMA kernel and the generic nb_conv2d_f32 (alex's 11 x 11 stride-4 and 5 x 5 layers, and the zero-stuffed
backward of perceptual._conv_input_grad with every right / bottom remainder) -- against float64 ``F.conv2d`` and its autograd on the
same float32 operands (tests/lpips_refs.py: LAYER_CASES, layer_reference, layer_bounds).

Layer by layer because a convolution and its input gradient are linear: no ReLU or pool decision is involved, and the pointwise
kernels between them are held exactly by test_hip_lpips.py.  The operands are what LPIPS feeds these kernels: 3 input channels (3 of a
16-channel chunk) or non-negative ReLU outputs with a third of zeros and per-sample scales; 3 output channels in the first layer's
input gradient (the ``tf`` pack padded from 3 to 64); pool-routed gradients that are three-quarters exact zeros, scaled by 1 / (h w)
and per sample (one all-zero); one power-of-two range scale per tensor for all of it.

Each case runs with ops.TRAIN_SPLIT_F16 on and off and declares its split-path branches (tests/split_branches.py): with the flag on the
recorded set equals the declared one, with it off no split token runs.  The forward is ``ops.conv2d`` under ``no_grad`` as
_LpipsHip.forward calls it, the input gradient is perceptual._conv_input_grad itself.  Bounds: the derived ones of
test_hip_train_grads_f64.py (lpips_refs.layer_bounds); nothing is measured.  Zeroing one channel of the float64 reference's input moves
the result by >= 20 bounds, an all-zero sample gives exact zeros, two launches give the same bytes, and the operands -- the buffers this
test allocates, between sentinel guards as in test_hip_lpips.py -- are left as they were; the results are allocated by ops.conv2d: their
shape is checked, and that every element is finite."""
import pytest
import torch

import lpips_refs as lr
import split_branches
from brushstroke_engine_amd import ops, perceptual
from test_hip_lpips import Guarded
from test_hip_step_kernels import within

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(params=[True, False], ids=["split_f16", "fp32"])
def mode(request, monkeypatch):
    """Sets ops.TRAIN_SPLIT_F16 and records the split-path branches that run; the flag is restored on the way out."""
    split = request.param
    rec = split_branches.record(monkeypatch)
    with split_branches.flags(split, names=("TRAIN_SPLIT_F16",)):
        yield split, rec


class _Net:
    """What perceptual._conv_input_grad reads of an LPIPS object: the layer's weight and, for a strided layer, the backward's kernel
    as LPIPS.__init__ keeps it."""

    def __init__(self, w, stride):
        self.weights = {0: w}
        self.weights_tf = {0: w.transpose(0, 1).flip([2, 3]).contiguous()} if stride != 1 else {}


def _guarded(t):
    g = Guarded(t.numel())
    g.view.copy_(t.reshape(-1).to(DEV))
    return g, g.view.view(t.shape)


def _report(what, got, want, tol):
    err = (got.detach().double().cpu() - want).abs()
    tol = tol.expand_as(err)
    ratio = torch.where(tol > 0, err / tol.clamp_min(1e-300), torch.where(err > 0, float("inf"), 0.0).double())     # (a zero bound: exact zeros)
    print(f"[lpips trunk] {what}: max err {float(err.max()):.3g}, worst err/bound {float(ratio.max()):.3g}")


@pytest.mark.parametrize("case", lr.LAYER_CASES, ids=lr.LAYER_IDS)
def test_trunk_layer_against_float64(mode, case):
    name, n, ci, co, h, w_, k, s, p, fwd_declared, bwd_declared = case
    flag, rec = mode
    label = f"{name} {'split_f16' if flag else 'fp32'}"
    ref = lr.layer_reference(case)
    ho, wo = lr.layer_out_size(h, k, s, p), lr.layer_out_size(w_, k, s, p)
    guards, (x, w, d) = zip(*[_guarded(ref[key]) for key in ("x", "w", "d")])
    net, lay = _Net(w, s), perceptual._Layer(0, s, p, None, 0)
    with torch.no_grad():
        y = ops.conv2d(x, w, stride=s, padding=p)
        torch.cuda.synchronize()
        ran_fwd = set(rec)
        rec.clear()
        dx = perceptual._conv_input_grad(d, net, lay, (n, ci, h, w_))
        torch.cuda.synchronize()
        ran_bwd = set(rec)
        y2 = ops.conv2d(x, w, stride=s, padding=p)
        dx2 = perceptual._conv_input_grad(d, net, lay, (n, ci, h, w_))
        torch.cuda.synchronize()
    print(f"[lpips trunk] {label}: forward ran {sorted(ran_fwd)}, input gradient ran {sorted(ran_bwd)}")
    split_branches.check(flag, ran_fwd, fwd_declared, f"{label} forward")
    split_branches.check(flag, ran_bwd, bwd_declared, f"{label} input gradient")
    assert tuple(y.shape) == (n, co, ho, wo) and tuple(dx.shape) == (n, ci, h, w_), (label, tuple(y.shape), tuple(dx.shape))
    assert y.dtype == torch.float32 and dx.dtype == torch.float32
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(dx).all()), f"{label}: a result that is not finite"
    assert torch.equal(y, y2) and torch.equal(dx, dx2), f"{label}: two launches differ"
    for g, key in zip(guards, ("x", "w", "d")):                            # the operands and what lies around them: untouched
        assert g.intact() and torch.equal(g.view.cpu(), ref[key].reshape(-1)), f"{label}: operand {key} or its guards were written"
    t_y = lr.layer_bounds(case, ref, flag and bool(fwd_declared))[0]
    t_dx = lr.layer_bounds(case, ref, flag and bool(bwd_declared))[1]
    for what, want, bad, tol in (("y", ref["y"], ref["y_bad"], t_y), ("dx", ref["dx"], ref["dx_bad"], t_dx)):
        moved = float((want - bad).abs().max())
        assert moved >= lr.CATCH_FACTOR * float(tol.max()), f"{label} {what}: a zeroed channel moves it by {moved:.3g}, bound {float(tol.max()):.3g}"
    _report(f"{label} y", y, ref["y"], t_y)
    _report(f"{label} dx", dx, ref["dx"], t_dx)
    within(y, ref["y"], t_y, f"{label} y")
    within(dx, ref["dx"], t_dx, f"{label} dx")
    zero = [i for i in range(n) if float(ref["d"][i].abs().max()) == 0.0]
    assert (n < 4) == (not zero)                                           # (dy_scales: an all-zero sample where n >= 4)
    for i in zero:
        assert float(dx[i].abs().max()) == 0.0, f"{label}: the all-zero sample {i} gives dx {float(dx[i].abs().max())}"
