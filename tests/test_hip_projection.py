"""GPU: the projection kernels (csrc/nb_projection.hip) against the float64 statement of tests/projection_refs.py at the smallest
shapes that can go wrong, the autograd Function around them against ``projection.loss_torch``, and ``projection.BrushProjector`` on the
HIP generator: route "hip" against route "torch" from the same state, and short runs whose results paint.

Bound of every kernel quantity (clarity_refs.bound): BOUND_FACTOR x the error of the float32 torch route on the same device tensors
against float64 -- the kernels sum in another order -- plus ULP_FLOOR float32 ulps of the value.  Masks and counts are compared
exactly (projection_refs.drawings keeps every blur value away from the thresholds).  Outputs sit between sentinel guards, ``uvs`` is a
channel slice of a NaN-filled wider tensor, ``img`` starts one float behind a 16-byte boundary (which sends the call down the
pixel-by-pixel path; the aligned variant of each case takes the 16-byte path where r * r allows), two launches give the same bytes,
and row 1 of a k = 2 launch is the k = 1 launch on that row."""
import numpy as np
import pytest
import torch

import clarity_refs as cr
import projection_refs as pr
from brushstroke_engine_amd import _lib, config as cfgmod, encoder as encmod, formats, painting, projection, weights as wmod

pytestmark = pytest.mark.gpu
GUARD = 64
DEV = "cuda"


class Guarded:
    """A device buffer of ``numel`` elements between two guards of a sentinel value; ``intact()`` after the launches."""

    def __init__(self, numel, dtype=torch.float32, sentinel=77, guard=GUARD):
        self.buf = torch.full([numel + 2 * guard], sentinel, dtype=dtype, device=DEV)
        self.view, self.guard, self.sentinel = self.buf[guard:guard + numel], guard, sentinel

    def intact(self):
        return bool((self.buf[:self.guard] == self.sentinel).all()) and bool((self.buf[-self.guard:] == self.sentinel).all())


def _st():
    return torch.cuda.current_stream().cuda_stream


def _ptr(x):
    return None if x is None else x.data_ptr()


def _stride(x):
    return 0 if x is None else x.stride(0)


def _within(got, want, bnd, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err = np.abs(got - want)
    worst = int(np.argmax(err - bnd))
    print(f"[projection] {what}: max err {err.max():.3g}, smallest bound {np.min(bnd):.3g}, worst err/bound {(err / np.maximum(bnd, 1e-300)).max():.3g}")
    assert np.all(np.isfinite(got)) and np.all(err <= bnd), (what, err.reshape(-1)[worst], np.broadcast_to(bnd, err.shape).reshape(-1)[worst])


def _dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


# ------------------------------------------------------------------------------------------------
# masks
# ------------------------------------------------------------------------------------------------
def _launch_masks(blur, target, k, b, r):
    n = k * b
    mask, counts = Guarded(n * r * r, torch.uint8), Guarded(2 * k, torch.int32)
    color, parts = Guarded(3 * k), Guarded(n * _lib.NB_PROJECTION_PARTS * 8)
    _lib.check(_lib.lib().nb_projection_masks_f32(blur.data_ptr(), target.data_ptr(), target.stride(0), k, b, r, mask.view.data_ptr(), counts.view.data_ptr(),
                                                  color.view.data_ptr(), parts.view.data_ptr(), _st()), "projection_masks")
    torch.cuda.synchronize()
    assert all(g.intact() for g in (mask, counts, color, parts))
    return mask.view.view(n, r, r).cpu().numpy(), counts.view.view(k, 2).cpu().numpy(), color.view.view(k, 3).cpu().numpy()


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset"])
@pytest.mark.parametrize("r,b,k", [(8, 1, 1), (20, 3, 2), (64, 3, 2), (64, 1, 1)])
def test_masks_entry(r, b, k, offset):
    """The chain nb_eval_masks_f32 -> nb_projection_masks_f32 on drawings, against masks from a float64 double blur: equal exactly.
    At r = 8 no pixel is four pixels from the border, so nothing is background: counts 0 and a zero colour."""
    n = k * b
    geom = pr.drawings(r, n, seed=r + n)
    rs = np.random.RandomState(r)
    flat = torch.full([n * 4 * r * r + 8], float("nan"), dtype=torch.float32, device=DEV)
    target = flat[offset:offset + n * 4 * r * r].view(n, 4, r, r)[:, :3]                    # a sample stride of 4 r r
    target.copy_(_dev(np.tanh(rs.randn(n, 3, r, r)).astype(np.float32)))
    g = _dev(geom[:, 0])
    blur, scratch_mask = torch.empty_like(g), torch.empty([n, r, r], dtype=torch.uint8, device=DEV)
    cnt = torch.empty([2, n], dtype=torch.int32, device=DEV)
    _lib.check(_lib.lib().nb_eval_masks_f32(g.data_ptr(), n, r, blur.data_ptr(), scratch_mask.data_ptr(), cnt[0].data_ptr(), cnt[1].data_ptr(), _st()), "eval_masks")
    got = _launch_masks(blur, target, k, b, r)
    again = _launch_masks(blur, target, k, b, r)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(got, again))
    mask64, counts64, color64 = pr.masks_f64(geom, target.cpu(), k)
    assert np.array_equal(got[0], mask64) and np.array_equal(got[1], counts64)
    fg, bg = projection.conservative_masks_torch(_dev(geom))
    color32 = projection.masked_color_torch(target, bg, k).cpu().numpy()
    _within(got[2], color64, cr.bound(color32, color64), "bg_color")
    if r == 8:
        assert np.all(got[1][:, 1] == 0) and np.all(got[2] == 0.0)
    elif r == 64:
        assert got[1].min() >= 37                                          # (every exemplar has both kinds of pixels)
    if k == 2:
        one = _launch_masks(blur[b:], target[b:], 1, b, r)
        assert one[0].tobytes() == got[0][b:].tobytes() and one[1].tobytes() == got[1][1:].tobytes() and one[2].tobytes() == got[2][1:].tobytes()
    # the wrapper is this chain
    m, c, col = projection.projection_masks_hip(_dev(geom), target, k)
    assert np.array_equal(m.cpu().numpy(), got[0]) and np.array_equal(c.cpu().numpy(), got[1]) and col.cpu().numpy().tobytes() == got[2].tobytes()


# ------------------------------------------------------------------------------------------------
# loss
# ------------------------------------------------------------------------------------------------
def _loss_views(c, offset):
    """The case's tensors on the device: uvs as channels 1..3 of a NaN-filled [n,5,r,r] tensor, img (or, with the composite, bg_image
    or target) ``offset`` floats behind a 16-byte boundary, the rest dense."""
    n, r = c["k"] * c["b"], c["r"]
    big = torch.full([n, 5, r, r], float("nan"), dtype=torch.float32, device=DEV)
    big[:, 1:4] = _dev(c["uvs"])

    def shifted(x):
        flat = torch.full([n * 3 * r * r + 8], float("nan"), dtype=torch.float32, device=DEV)
        v = flat[offset:offset + n * 3 * r * r].view(n, 3, r, r)
        v.copy_(_dev(x))
        return v
    img, target, bgi = _dev(c["img"]), _dev(c["target"]), _dev(c["bg_image"])
    if not c["composite"]:
        img = shifted(c["img"])
    elif bgi is not None:
        bgi = shifted(c["bg_image"])
    else:
        target = shifted(c["target"])
    return dict(uvs=big[:, 1:4], colors=_dev(c["colors"]), img=img, target=target, bg_image=bgi, bg_color=_dev(c["bg_color"]), mask=_dev(c["mask"]),
                counts=_dev(c["counts"]))


def _launch_loss(v, k, b, r, composite, w, d_synth=None, gscale=None):
    n = k * b
    lib = _lib.lib()
    out, parts, synth = Guarded(3 * k), Guarded(n * _lib.NB_PROJECTION_PARTS * 16), Guarded(n * 3 * r * r)
    d_uvs, d_img, d_col = Guarded(n * 3 * r * r), Guarded(n * 3 * r * r), Guarded(n * 9)
    common = (v["uvs"].data_ptr(), v["uvs"].stride(0), _ptr(v["colors"]) if composite else None, None if composite else v["img"].data_ptr(),
              0 if composite else v["img"].stride(0), v["target"].data_ptr(), v["target"].stride(0), _ptr(v["bg_image"]) if composite else None,
              _stride(v["bg_image"]), v["bg_color"].data_ptr(), v["mask"].data_ptr(), v["counts"].data_ptr())
    _lib.check(lib.nb_projection_loss_f32(*common, k, b, r, int(composite), w[0], w[1], synth.view.data_ptr() if composite else None, out.view.data_ptr(),
                                          parts.view.data_ptr(), _st()), "projection_loss")
    _lib.check(lib.nb_projection_loss_bwd_f32(*common, _ptr(d_synth), _ptr(gscale), k, b, r, int(composite), w[0], w[1], d_uvs.view.data_ptr(),
                                              None if composite else d_img.view.data_ptr(), d_col.view.data_ptr() if composite else None,
                                              parts.view.data_ptr() if composite else None, _st()), "projection_loss_bwd")
    torch.cuda.synchronize()
    assert all(g.intact() for g in (out, parts, synth, d_uvs, d_img, d_col))
    sent = lambda g: bool((g.view == g.sentinel).all())
    assert (sent(d_img) and not sent(synth)) if composite else (sent(synth) and sent(d_col))   # what is not asked for is not written
    return dict(out=out.view.view(k, 3).cpu().numpy(), synth=synth.view.view(n, 3, r, r).cpu().numpy(), d_uvs=d_uvs.view.view(n, 3, r, r).cpu().numpy(),
                d_img=d_img.view.view(n, 3, r, r).cpu().numpy(), d_colors=d_col.view.view(n, 3, 3).cpu().numpy())


def _check_loss_case(c, offset, with_d_synth, with_gscale):
    k, b, r, composite, w = c["k"], c["b"], c["r"], c["composite"], c["weights"]
    n = k * b
    v = _loss_views(c, offset)
    gscale = torch.tensor([1.0, 0.25][:k], dtype=torch.float32, device=DEV) if with_gscale else None
    d_synth = _dev((np.random.RandomState(5).randn(n, 3, r, r) * 1e-3).astype(np.float32)) if with_d_synth else None
    got = _launch_loss(v, k, b, r, composite, w, d_synth, gscale)
    again = _launch_loss(v, k, b, r, composite, w, d_synth, gscale)
    keys = ("out", "synth", "d_uvs", "d_colors") if composite else ("out", "d_uvs", "d_img")
    assert all(got[x].tobytes() == again[x].tobytes() for x in keys)
    # float64 statement, and the float32 torch route on the same device tensors
    host = lambda x: None if x is None else x.cpu().numpy()
    args64 = (c["uvs"], c["colors"], c["img"], c["target"], c["bg_image"], c["bg_color"], c["mask"], k, composite, w)
    out64, synth64 = pr.loss_f64(*args64)
    du64, di64, dc64 = pr.loss_bwd_f64(*args64, host(d_synth), host(gscale))
    m = v["mask"].to(torch.int64).unsqueeze(1)
    fg, bg = ((m >> 1) & 1).bool(), (m & 1).bool()
    u32, c32, i32 = v["uvs"].clone().requires_grad_(True), v["colors"].clone().requires_grad_(True), v["img"].clone().requires_grad_(True)
    out32, synth32 = projection.loss_torch(u32, c32, i32, v["target"], v["bg_image"] if composite else None, v["bg_color"], fg, bg, k, composite, w)
    obj = (out32[:, 2] * (gscale if gscale is not None else 1.0)).sum()
    if d_synth is not None:                                                # (without the composite synth IS img: the upstream gradient reaches d_img)
        obj = obj + (synth32 * d_synth).sum()
    obj.backward()
    what = f"r{r} b{b} k{k} comp{int(composite)} ds{int(with_d_synth)} gs{int(with_gscale)}"
    _within(got["out"], out64.numpy(), cr.bound(out32.detach().cpu().numpy(), out64.numpy()), what + " out")
    _within(got["d_uvs"], du64, cr.bound(u32.grad.cpu().numpy(), du64), what + " d_uvs")
    h, wd = r // 2, r // 3
    if composite:
        _within(got["synth"], synth64.numpy(), cr.bound(synth32.detach().cpu().numpy(), synth64.numpy()), what + " synth")
        _within(got["d_colors"], dc64, cr.bound(c32.grad.cpu().numpy(), dc64), what + " d_colors")
        assert np.array_equal(got["synth"][:, :, :h, :wd], host(v["target"])[:, :, :h, :wd])     # the region where synth IS the background
        if d_synth is None:                                                # sign(0) = 0 there: a foreground pixel's uvs[2] gets nothing
            fgm = c["mask"][:, :h, :wd] == 2
            assert fgm.any() and np.all(got["d_uvs"][:, 2, :h, :wd][fgm] == 0.0) and np.any(got["d_uvs"][:, :2] != 0.0)
    else:
        _within(got["d_img"], di64, cr.bound(i32.grad.cpu().numpy(), di64), what + " d_img")
        assert np.all(got["d_uvs"][:, :2] == 0.0)                          # exactly
        if d_synth is None:                                                # sign(0) = 0 where target equals img
            assert np.all(got["d_img"][:, :, :h, :wd] == 0.0) and np.any(got["d_img"] != 0.0)
        else:                                                              # ... so there the upstream gradient passes through unchanged
            assert np.array_equal(got["d_img"][:, :, :h, :wd], host(d_synth)[:, :, :h, :wd])
    if k == 2:                                                             # row 1 alone: the same bytes
        n1 = slice(b, 2 * b)
        v1 = {key: (None if x is None else (x[1:] if key in ("bg_color", "counts") else x[n1])) for key, x in v.items()}
        one = _launch_loss(v1, 1, b, r, composite, w, None if d_synth is None else d_synth[n1], None if gscale is None else gscale[1:])
        assert one["out"].tobytes() == got["out"][1:].tobytes()
        assert all(one[x].tobytes() == got[x][n1].tobytes() for x in keys[1:])
    return got


@pytest.mark.parametrize("with_gscale", [False, True], ids=["gs0", "gs1"])
@pytest.mark.parametrize("with_d_synth", [False, True], ids=["ds0", "ds1"])
@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset"])
@pytest.mark.parametrize("composite,bg_image", [(True, False), (True, True), (False, False)], ids=["colour", "image", "plain"])
@pytest.mark.parametrize("r,b,k", pr.LOSS_CASES, ids=[f"r{r}_b{b}_k{k}" for r, b, k in pr.LOSS_CASES])
def test_loss_entries(r, b, k, composite, bg_image, offset, with_d_synth, with_gscale):
    """d_synth and gscale are each given or null on their own; d_synth is also given without the composite, where it reaches d_img."""
    c = pr.loss_case(r, b, k, composite=composite, bg_image=bg_image, no_fg_patch=b > 1)
    _check_loss_case(c, offset, with_d_synth, with_gscale)


@pytest.mark.parametrize("composite", [True, False])
def test_exemplar_without_foreground_has_item_and_gradient_zero(composite):
    c = pr.loss_case(20, 2, 2, composite=composite, no_fg_exemplar=True)
    assert c["counts"][1, 0] == 0 and c["counts"][0, 0] > 0
    got = _check_loss_case(c, 0, with_d_synth=False, with_gscale=True)
    assert got["out"][1, 0] == 0.0 and got["out"][1, 2] == np.float32(c["weights"][1]) * got["out"][1, 1]
    if composite:
        assert np.all(got["d_colors"][2:] == 0.0) and np.all(got["d_uvs"][2:, :2] == 0.0)
    else:
        assert np.all(got["d_img"][2:] == 0.0)
    # no background either: everything of that exemplar is zero
    c["mask"][2:] = 0
    c["counts"] = pr.counts_of(c["mask"], 2)
    got = _check_loss_case(c, 0, with_d_synth=False, with_gscale=False)
    assert np.all(got["out"][1] == 0.0) and np.all(got["d_uvs"][2:] == 0.0)


class _Leaf:
    """A leaf tensor and a NON-CONTIGUOUS view of it that holds ``x``.  'slice': the view is indices 1..C of a NaN-filled axis of C + 2 (a
    channel slice of a wider tensor for [n,3,r,r]: dense planes, a sample stride above 3 r r, read in place by the entries).  'transposed':
    the leaf holds x with its last two axes swapped and the view swaps them back (planes that are not dense: the wrapper has to copy)."""

    def __init__(self, x, layout, dtype, requires_grad=True):
        x = _dev(x).to(dtype)
        self.layout, self.axis = layout, 1 if x.dim() == 4 else 2
        if layout == "slice":
            shape = list(x.shape)
            shape[self.axis] += 2
            self.leaf = torch.full(shape, float("nan"), dtype=dtype, device=DEV)
            self.leaf.narrow(self.axis, 1, x.shape[self.axis]).copy_(x)
            self.leaf.requires_grad_(requires_grad)
            self.view = self.leaf.narrow(self.axis, 1, x.shape[self.axis])
        else:
            self.leaf = x.transpose(-1, -2).contiguous().requires_grad_(requires_grad)
            self.view = self.leaf.transpose(-1, -2)
        assert not self.view.is_contiguous() and torch.equal(self.view.detach(), x)

    def grad(self):
        """The gradient that arrived at the view's elements, as numpy; what lies outside the view got none."""
        g = self.leaf.grad
        if g is None:
            return None
        if self.layout == "transposed":
            return g.transpose(-1, -2).cpu().numpy()
        n = g.shape[self.axis]
        assert bool((g.narrow(self.axis, 0, 1) == 0).all()) and bool((g.narrow(self.axis, n - 1, 1) == 0).all())
        return g.narrow(self.axis, 1, n - 2).cpu().numpy()


@pytest.mark.parametrize("layout", ["slice", "transposed"])
@pytest.mark.parametrize("composite,bg_image", [(True, False), (True, True), (False, False)], ids=["colour", "image", "plain"])
def test_fused_loss_function_matches_torch_route(composite, bg_image, layout):
    """The autograd.Function around the entries with the stand-in perceptual item attached, on NON-CONTIGUOUS inputs: uvs, colors, img,
    target and bg_image are views of leaves -- slices with a sample stride above 3 r r, which the entries read in place, or transposed
    views, which the wrapper copies -- and the gradients are compared where they arrive, at the leaves.  Bound against float64 as for
    the entries."""
    c = pr.loss_case(20, 3, 2, composite=composite, bg_image=bg_image)
    mask, counts = _dev(c["mask"]), _dev(c["counts"])
    m = mask.to(torch.int64).unsqueeze(1)
    fg, bg = ((m >> 1) & 1).bool(), (m & 1).bool()
    gs = torch.tensor([1.0, 0.25], device=DEV)
    grads = {}
    for route in ("hip", "torch", "f64"):
        dt = torch.float64 if route == "f64" else torch.float32
        u, col, im = (_Leaf(c[x], layout, dt) for x in ("uvs", "colors", "img"))
        tg = _Leaf(c["target"], layout, dt, requires_grad=False).view
        bgi = None if c["bg_image"] is None else _Leaf(c["bg_image"], layout, dt, requires_grad=False).view
        bgc = _dev(c["bg_color"]).to(dt)
        if layout == "slice":
            assert u.view.stride(0) == 5 * 400 and tg.stride(0) == 5 * 400 and u.view.stride(1) == 400
        if route == "hip":
            total, items, synth = projection.fused_projection_loss(u.view, col.view, im.view, tg, bgi, bgc, mask, counts, 2, composite, c["weights"])
            assert not items.requires_grad
        else:
            out, synth = projection.loss_torch(u.view, col.view, im.view, tg, bgi, bgc, fg, bg, 2, composite, c["weights"])
            total, items = out[:, 2], out[:, :2].detach()
        perc = pr.stand_in_perceptual(tg, synth).reshape(2, 3).mean(dim=1)
        ((total + 3.0 * perc) * gs.to(dt)).sum().backward()
        grads[route] = [total.detach().cpu().numpy(), items.cpu().numpy(), u.grad(), col.grad() if composite else im.grad()]
        assert (im.grad() is None) if composite else (col.grad() is None)
    for name, g, t32, f64 in zip(("total", "items", "d_uvs", "d_colors" if composite else "d_img"), grads["hip"], grads["torch"], grads["f64"]):
        _within(g, f64, cr.bound(t32, f64), f"function {layout} comp{int(composite)} img{int(bg_image)} {name}")


# ------------------------------------------------------------------------------------------------
# the projector on the HIP generator
# ------------------------------------------------------------------------------------------------
def test_gradient_arena_hip_route_against_torch_route():
    """From identical state: the generator is the same, only the loss and the regulariser differ.  Bound as above, the float32 torch
    route's error being measured against the float64 run on the oracle (CPU)."""
    from brushstroke_engine_amd.training import TrainableGenerator
    cfg, k, b = cfgmod.tiny_config(32), 2, 3
    sd = wmod.random_state_dict(cfg, 5)
    T = TrainableGenerator(cfg, sd, DEV).requires_grad_(False)
    enc = cr.StandInEncoder(cfg)
    exs = [pr.exemplar(32, b, seed=31), pr.exemplar(32, b, seed=32)]
    kw = dict(w_plus=True, with_composite=True, l1_fg_weight=0.7, bg_weight=1.3, perceptual=pr.stand_in_perceptual, w_avg=np.zeros([1, 1, cfg.w_dim]), w_std=1.0)
    lo = projection.BrushProjector(T, enc, route="torch", **kw).layout
    rs = np.random.RandomState(6)
    arena = rs.randn(k, lo.p).astype(np.float32)
    w_noise = 0.05 * rs.randn(k, *lo.w_shape).astype(np.float32)
    res = {}
    for route in ("hip", "torch"):
        p = projection.BrushProjector(T, enc, route=route, **kw)
        out = p.loss_and_grad(_dev(arena), _dev(w_noise), p.prepare(exs))
        res[route] = [x.cpu().numpy() for x in out]
    p64 = projection.BrushProjector(pr.OracleGen(cfg, sd, torch.float64), enc, route="torch", device="cpu", **kw)
    fix = p64.prepare([tuple(None if x is None else x.double() for x in e) for e in exs])
    for key in ("target", "geom", "bg_color"):
        fix[key] = fix[key].double()
    fix["feats"] = [f.double() for f in fix["feats"]]
    want = [x.numpy() for x in p64.loss_and_grad(torch.from_numpy(arena.astype(np.float64)), torch.from_numpy(w_noise.astype(np.float64)), fix)]
    for name, j in (("gradient arena", 0), ("items", 1), ("reg", 2), ("criterion", 3)):
        _within(res["hip"][j], want[j], cr.bound(res["torch"][j], want[j]), f"projector {name}")
    assert np.abs(want[0][:, lo.nw:]).max() > 0 and np.abs(want[0][:, :lo.nw]).max() > 0


def _paints(cfg, sd, enc, entry, drawing):
    """The result paints through PaintingHelper with its noise set: the same bytes as a checkpoint that holds those planes."""
    from brushstroke_engine_amd.networks import Generator
    lib = formats.WBrushLibrary({"x": entry})
    opts = painting.GanBrushOptions()
    lib.set_style("x", opts)
    geom = drawing[:, :, None]
    with torch.no_grad():
        img = painting.PaintingHelper(painting.TileOps(Generator(cfg, sd).to(DEV), enc), batch=2).paint_image(geom, opts, crop_margin=10)
        sd2 = dict(sd)
        sd2.update({"synthesis." + n: v.numpy() for n, v in entry["noise"].items()})
        plain = painting.GanBrushOptions()
        plain.set_style_w(entry["w"].expand(1, cfg.num_ws, cfg.w_dim).contiguous(), "x")
        held = painting.PaintingHelper(painting.TileOps(Generator(cfg, sd2).to(DEV), enc), batch=2).paint_image(geom, plain, crop_margin=10)
    assert img.shape[:2] == drawing.shape and np.array_equal(img, held)


@pytest.fixture(scope="module")
def shipped():
    cfg = cfgmod.style1_config(128)
    sd, esd = wmod.random_state_dict(cfg, seed=0), encmod.random_encoder_state_dict(5)
    exs = {"chalk": pr.exemplar(128, 2, seed=41, with_positions=True), "oil": pr.exemplar(128, 2, seed=42, with_positions=True)}
    return cfg, sd, encmod.HipGeometryEncoder(esd), exs


def test_three_step_run_paints(shipped):
    """Route "hip" at the shipped shapes (style1_config(128), the HIP encoder), K = 2, B = 2, composite and positions."""
    from brushstroke_engine_amd.training import TrainableGenerator
    cfg, sd, enc, exs = shipped
    T = TrainableGenerator(cfg, sd, DEV)
    p = projection.BrushProjector(T, enc.encode, num_steps=3, w_plus=True, with_composite=True, with_positions=True, l1_fg_weight=1.0, bg_weight=0.5,
                                  w_avg_samples=64)
    assert p.route == "hip"
    seen = []
    out = p.project(exs, brushes_per_pass=2, seed=1, on_step=lambda ids, step, lr, items, reg: seen.append((step, items.cpu().numpy(), reg.cpu().numpy())))
    assert sorted(out) == ["chalk", "oil"] and len(seen) == 3 and all(np.isfinite(s[1]).all() and np.isfinite(s[2]).all() for s in seen)
    assert all(q.requires_grad for q in T.parameters()) and all(q.grad is None for q in T.parameters())
    lo = p.layout
    for sid, e in out.items():
        assert tuple(e["w"].shape) == (1, cfg.num_ws, cfg.w_dim) and sorted(e["noise"]) == sorted(lo.names) and bool(torch.isfinite(e["w"]).all())
        assert e["step"] == 2 and tuple(e["bg"].shape) == (3,) and bool(torch.isfinite(e["bg"]).all())
        for name, r in zip(lo.names, lo.res):
            n = e["noise"][name].double()
            assert tuple(n.shape) == (r, r) and bool(torch.isfinite(n).all())
            assert abs(float(n.mean())) <= 8 * cr.EPS32 and abs(float((n * n).mean()) - 1) <= cr.mean_square_tol(r), (sid, name)
        assert set(p.history[sid]) == {"first", "last"} and set(p.history[sid]["last"]) == {"l1", "bg", "noise_reg"}
    _paints(cfg, sd, enc, out["chalk"], (exs["chalk"][1][0, 0].numpy() * 255).astype(np.uint8))


def test_three_step_run_in_w_without_noise_paints(shipped):
    from brushstroke_engine_amd.training import TrainableGenerator
    cfg, sd, enc, exs = shipped
    p = projection.BrushProjector(TrainableGenerator(cfg, sd, DEV), enc.encode, num_steps=3, w_plus=False, optimize_noise=False, with_composite=True,
                                  with_positions=True, l1_fg_weight=1.0, bg_weight=0.5, w_avg_samples=64)
    out = p.project(exs, brushes_per_pass=2, seed=1)
    for sid, e in out.items():
        assert tuple(e["w"].shape) == (1, 1, cfg.w_dim) and e["noise"] == {} and bool(torch.isfinite(e["w"]).all())
    assert float((out["chalk"]["w"] - out["oil"]["w"]).abs().max()) > 0
    _paints(cfg, sd, enc, out["oil"], (exs["oil"][1][0, 0].numpy() * 255).astype(np.uint8))
