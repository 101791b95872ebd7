"""nb_brush_noise_build_f32 on the GPU, bit for bit against numpy: the one launch that writes every layer of a brush noise set
(noise_const replacement and its transpose; a copy, or the float32 lerp of two brushes).  Every layer of style1_config(256) goes
through a single launch: 13 layers, res 4 ... 256, five of them smaller than the 32 x 32 tile, up to 64 tiles per layer.  One case
runs the 15 layers of style1_config(512) the same way."""
import ctypes

import numpy as np
import pytest
import torch

from brushstroke_engine_amd import _lib, config as cfgmod

pytestmark = pytest.mark.gpu

RES = [s.block_res for s in cfgmod.style1_config(256).layers]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def images():
    """Two host images per layer: a, b (never modified)."""
    rs = np.random.RandomState(20)
    return [(rs.randn(r, r).astype(np.float32), rs.randn(r, r).astype(np.float32)) for r in RES]


def _dev_image(host, dev, offset_floats=0):
    """A device copy of `host` starting `offset_floats` floats behind a fresh allocation (allocations are 256-byte aligned)."""
    flat = torch.empty([host.size + offset_floats], dtype=torch.float32, device=dev)
    view = flat[offset_floats:].view(host.shape)
    view.copy_(torch.from_numpy(host))
    return view


def _build(layers, wa, wb, dev):
    arr = (_lib.NbBrushNoiseLayer * len(layers))()
    for L, (a, b, dst, dst_t, res) in zip(arr, layers):
        L.a, L.b, L.dst, L.dst_t, L.res = a.data_ptr(), None if b is None else b.data_ptr(), dst.data_ptr(), dst_t.data_ptr(), res
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().nb_brush_noise_build_f32(arr, len(layers), wa, wb, torch.cuda.current_stream(dev).cuda_stream), "build")
    torch.cuda.synchronize(dev)


def _lerp(a, b, alpha):
    """What numpy gives for `a * alpha + b * (1 - alpha)` on float32 arrays: the weights rounded to float32, two rounded
    products, one rounded sum."""
    return a * np.float32(alpha) + b * np.float32(1 - alpha)


def _fresh(res, dev, offset=0):
    t = torch.full([res * res + offset], float("nan"), dtype=torch.float32, device=dev)
    return t[offset:].view(res, res)


def test_layout_is_every_layer_from_4_to_256():
    assert len(RES) == 13 and RES[0] == 4 and RES[-1] == 256 and sorted(set(RES)) == [4, 8, 16, 32, 64, 128, 256]


def test_fifteen_layers_in_one_launch(dev):
    """style1_config(512): 15 layers, 256 tiles in the largest; every other layer lerps."""
    res = [s.block_res for s in cfgmod.style1_config(512).layers]
    assert len(res) == 15 and res[-1] == 512
    rs = np.random.RandomState(21)
    host = [(rs.randn(r, r).astype(np.float32), rs.randn(r, r).astype(np.float32)) for r in res]
    layers = [(_dev_image(a, dev), _dev_image(b, dev) if i % 2 else None, _fresh(r, dev), _fresh(r, dev), r)
              for i, ((a, b), r) in enumerate(zip(host, res))]
    _build(layers, float(np.float32(0.7)), float(np.float32(1 - 0.7)), dev)
    for i, ((a, b), (_, _, dst, dst_t, r)) in enumerate(zip(host, layers)):
        want = _lerp(a, b, 0.7) if i % 2 else a
        assert np.array_equal(dst.cpu().numpy(), want) and np.array_equal(dst_t.cpu().numpy(), want.T), (i, r)


def test_copy_form(dev, images):
    layers = [(_dev_image(a, dev), None, _fresh(r, dev), _fresh(r, dev), r) for (a, _), r in zip(images, RES)]
    _build(layers, 1.0, 0.0, dev)
    for (a, _), (_, _, dst, dst_t, r) in zip(images, layers):
        assert np.array_equal(dst.cpu().numpy(), a), r
        assert np.array_equal(dst_t.cpu().numpy(), a.T), r


@pytest.mark.parametrize("alpha", [0.25, 0.7])
def test_lerp_form(dev, images, alpha):
    layers = [(_dev_image(a, dev), _dev_image(b, dev), _fresh(r, dev), _fresh(r, dev), r) for (a, b), r in zip(images, RES)]
    _build(layers, float(np.float32(alpha)), float(np.float32(1 - alpha)), dev)
    for (a, b), (_, _, dst, dst_t, r) in zip(images, layers):
        want = _lerp(a, b, alpha)
        assert np.array_equal(dst.cpu().numpy(), want), (r, float(np.abs(dst.cpu().numpy() - want).max()))
        assert np.array_equal(dst_t.cpu().numpy(), want.T), r


def test_mixed_table_aliased_dst_and_unaligned_pointers(dev, images):
    """Every other layer lerps, the rest copy; dst IS a (a reload in place); every pointer sits 4 bytes behind a 16-byte boundary."""
    alpha = 0.7
    layers = []
    for i, ((a, b), r) in enumerate(zip(images, RES)):
        a_dev = _dev_image(a, dev, 1)
        layers.append((a_dev, _dev_image(b, dev, 1) if i % 2 else None, a_dev, _fresh(r, dev, 1), r))
    assert all(t.data_ptr() % 16 == 4 for L in layers for t in L[:4] if t is not None)
    _build(layers, float(np.float32(alpha)), float(np.float32(1 - alpha)), dev)
    for i, ((a, b), (_, _, dst, dst_t, r)) in enumerate(zip(images, layers)):
        want = _lerp(a, b, alpha) if i % 2 else a
        assert np.array_equal(dst.cpu().numpy(), want), (i, r)
        assert np.array_equal(dst_t.cpu().numpy(), want.T), (i, r)


def test_single_res4_layer(dev, images):
    a, b = images[0]
    guard = torch.full([64], 7.0, dtype=torch.float32, device=dev)       # dst_t in the middle: nothing around it may change
    dst, dst_t = _fresh(4, dev), guard[24:40].view(4, 4)
    _build([(_dev_image(a, dev), _dev_image(b, dev), dst, dst_t, 4)], 0.25, 0.75, dev)
    want = _lerp(a, b, 0.25)
    assert np.array_equal(dst.cpu().numpy(), want) and np.array_equal(dst_t.cpu().numpy(), want.T)
    g = guard.cpu().numpy()
    assert np.all(g[:24] == 7.0) and np.all(g[40:] == 7.0)
