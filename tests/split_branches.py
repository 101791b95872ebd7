"""Recorder of the split-f16 branches that brushstroke_engine_amd.ops takes, shared by the GPU tests that declare their branches
(test_hip_train_grads_f64.py, test_hip_lpips_trunk_f64.py).

``record(monkeypatch)`` wraps ops._conv2d_launch, ops._split_f16_eligible, ops._s2_valid_h3_supported, ops._conv2d_s2_valid_h3,
ops.pack_conv_weight_h3_dev and the library's split weight-gradient entry, and returns the set that receives a token per branch:

  split_up1 / split_canvas        an up = 1 convolution on the split-f16 kernel: as it is / through ops._conv2d_launch's embedded canvas
  split_up2_w32 / split_up2_w16   an up = 2 convolution on the split-f16 kernels
  s2v_wide / s2v_narrow           nb_conv3x3_s2_valid_h3
  tf_pack                         the device weight pack of the transposed, tap-reversed weight
  wgrad_h3                        the split weight-gradient kernel
  off_split / s2_generic          a convolution that stays on the fp32 kernels (no split token)

``split_canvas`` is named by where the branch was entered -- ops._conv2d_launch given an image that is no power of two -- and not by
the canvas's size: a 31 x 31 image embeds into a 32 x 32 canvas, which is a power of two.  (An up = 1 convolution that reaches the
split kernel with a non-power-of-two image by another way is recorded as split_canvas too, as before.)"""
import contextlib
import threading

from brushstroke_engine_amd import ops

SPLIT_TOKENS = {"split_up1", "split_canvas", "split_up2_w32", "split_up2_w16", "s2v_wide", "s2v_narrow", "tf_pack", "wgrad_h3"}


def _is_pow2_image(h, w_):
    return ops._pow2(h) and ops._pow2(w_)


def record(monkeypatch):
    """Installs the wrappers (undone by ``monkeypatch``) and returns the set of recorded tokens."""
    rec = set()
    launch, elig, s2ok = ops._conv2d_launch, ops._split_f16_eligible, ops._s2_valid_h3_supported
    s2run, pack = ops._conv2d_s2_valid_h3, ops.pack_conv_weight_h3_dev
    lib = ops._lib.lib()
    wg = lib.nb_conv2d_wgrad_h3_ws
    entered = threading.local()                                          # (autograd runs the backward on a thread of its own)

    def w_launch(x, w, in_scale, out_scale, stride, padding):
        before = getattr(entered, "odd", False)
        entered.odd = not _is_pow2_image(x.shape[2], x.shape[3])
        try:
            return launch(x, w, in_scale, out_scale, stride, padding)
        finally:
            entered.odd = before

    def w_elig(n, h, w_, up):
        r = elig(n, h, w_, up)
        if r:
            canvas = getattr(entered, "odd", False) or not _is_pow2_image(h, w_)
            rec.add(("split_canvas" if canvas else "split_up1") if up == 1 else ("split_up2_w16" if w_ == 16 else "split_up2_w32"))
        else:
            rec.add("off_split")                                         # (a convolution that stays on the fp32 kernels)
        return r

    def w_wgrad(*args):
        rec.add("wgrad_h3")
        return wg(*args)

    def w_s2ok(n, ci, h, wd, kh, kw, stride, padding):
        r = s2ok(n, ci, h, wd, kh, kw, stride, padding)
        if not r and stride == 2:
            rec.add("s2_generic")
        return r

    def w_s2run(x, w, in_scale, out_scale):
        rec.add("s2v_wide" if ((x.shape[3] - 1) // 2) % 32 == 0 else "s2v_narrow")
        return s2run(x, w, in_scale, out_scale)

    def w_pack(weight, co_align=64, tf=False):
        if tf:
            rec.add("tf_pack")
        return pack(weight, co_align, tf)

    monkeypatch.setattr(ops, "_conv2d_launch", w_launch)
    monkeypatch.setattr(ops, "_split_f16_eligible", w_elig)
    monkeypatch.setattr(ops, "_s2_valid_h3_supported", w_s2ok)
    monkeypatch.setattr(ops, "_conv2d_s2_valid_h3", w_s2run)
    monkeypatch.setattr(ops, "pack_conv_weight_h3_dev", w_pack)
    monkeypatch.setattr(lib, "nb_conv2d_wgrad_h3_ws", w_wgrad)
    return rec


@contextlib.contextmanager
def flags(split, names=("TRAIN_SPLIT_F16", "WGRAD_SPLIT_F16")):
    """Sets the named ops flags to ``split``; restores them on the way out."""
    saved = [getattr(ops, nm) for nm in names]
    try:
        for nm in names:
            setattr(ops, nm, split)
        yield
    finally:
        for nm, v in zip(names, saved):
            setattr(ops, nm, v)


def check(split, rec, declared, what):
    """Flags on: the split-path branches that ran are exactly the declared ones.  Flags off: no split-path branch at all."""
    if split:
        ran = rec - {"off_split"}
        assert ran == set(declared), f"{what}: declared branches {sorted(declared)}, ran {sorted(ran)}"
    else:
        assert not (rec & SPLIT_TOKENS), f"{what}: split-f16 branches ran with the flags off: {sorted(rec & SPLIT_TOKENS)}"
