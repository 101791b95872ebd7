"""GPU: nb_noise_seeded_f32 (csrc/nb_noise_seeded.hip) through its C entry on small hand-built layer tables, against the numpy
restatement of its generator (tests/philox_ref.py: the same Philox integers, uniforms and Box-Muller in float64).

The bound, per pixel: |z - z64| <= 6 * 2^-23 * r64, with r64 = sqrt(-2 ln u1) the Box-Muller radius of the pixel's pair, and z == 0
where r64 == 0.  Derivation (u1, u2 and the trigonometric argument 2 u2 are exact in fp32, -2 * logf is a power-of-two scaling):
logf within 1 ulp is a relative error of 2^-23 of the logarithm, halved by the square root, plus the correctly rounded sqrtf's
2^-24: r within 2^-23 relative; sincospif within 2 ulp of a value <= 1: 2 * 2^-23 absolute, times r; the product's rounding 2^-24 r.
Sum 3.5 * 2^-23 r; the factor 6 leaves about 1.7x margin.  (The ulp figures are OpenCL's for log and sinpi / cospi, which the
device library follows; they could not be re-measured where this test was written.)  A wrong counter layout, key order or pair
order fails this by O(1), not by ulps; every identity between two launches (batch split, state pointer, strength) is bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

import philox_ref as pr
from brushstroke_engine_amd import _lib
from philox_ref import STAT_N, STAT_RES, STAT_SEEDS, check_statistics

pytestmark = pytest.mark.gpu
GUARD = 64                                     # canary floats on either side of every image buffer (keeps 16-byte alignment)
CANARY = -12345.0
TOL = 6.0 * 2.0 ** -23


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


def stream():
    return torch.cuda.current_stream().cuda_stream


class Table:
    """NbLayerDesc[] with one row per entry of `res` (None: a row without noise_out, like the ToRGB's), noise_strength NULL unless
    `strength` gives a [1] tensor per row; each image buffer [n_max, res, res] sits between canaries."""

    def __init__(self, res, n_max, dev, strength=None):
        self.res, self.n_max = list(res), n_max
        self.bufs = [None if r is None else torch.full([n_max * r * r + 2 * GUARD], CANARY, dtype=torch.float32, device=dev) for r in res]
        self.strength = strength or [None] * len(res)
        descs = (_lib.NbLayerDesc * len(res))()
        for d, r, b, s in zip(descs, self.res, self.bufs, self.strength):
            d.res = 0 if r is None else r
            d.noise_out = 0 if b is None else b.data_ptr() + 4 * GUARD
            d.noise_strength = 0 if s is None else s.data_ptr()
        self.dev_table = torch.from_numpy(np.frombuffer(bytes(descs), dtype=np.uint8).copy()).to(dev)
        self.max_res = max(r for r in self.res if r is not None)

    def run(self, first_layer, seed, offset, n, state=None, rows=None):
        lo, cnt = rows or (0, len(self.res))
        for b in self.bufs:
            if b is not None:
                b.fill_(CANARY)
        _lib.check(_lib.lib().nb_noise_seeded_f32(self.dev_table.data_ptr() + lo * ctypes.sizeof(_lib.NbLayerDesc), first_layer, cnt,
                                                  self.max_res, seed, offset, None if state is None else state.data_ptr(), n, stream()),
                   "noise_seeded")
        torch.cuda.synchronize()
        return [None if b is None else b.cpu().numpy() for b in self.bufs]

    def images(self, raw, i, n):
        """Row i's [n, res, res] images; asserts that nothing else of the buffer was written."""
        r = self.res[i]
        body = raw[i][GUARD:GUARD + self.n_max * r * r]
        assert (raw[i][:GUARD] == CANARY).all() and (raw[i][GUARD + self.n_max * r * r:] == CANARY).all(), f"row {i}: canary overwritten"
        assert (body[n * r * r:] == CANARY).all(), f"row {i}: samples past the batch written"
        return body[:n * r * r].reshape(n, r, r)


def check_against_reference(got, seed, offset, layer, what):
    """got [n, res, res] fp32 (no strength) vs the float64 restatement, within the module docstring's bound."""
    n, res = got.shape[0], got.shape[1]
    for k in range(n):
        z64, r64 = pr.seeded_noise(seed, offset, layer, k, res)
        g = got[k].astype(np.float64)
        assert np.isfinite(g).all(), f"{what}: sample {k} not finite"
        err = np.abs(g - z64)
        bad = err > TOL * r64
        assert not bad.any(), (f"{what}: sample {k}: {int(bad.sum())} of {bad.size} pixels outside 6 * 2^-23 r; worst "
                               f"{float((err / np.maximum(TOL * r64, 1e-300)).max()):.3g}x")
        assert (g[r64 == 0] == 0).all(), f"{what}: sample {k}: z != 0 where r == 0"


@pytest.mark.parametrize("res, n, seed, offset, layer", [
    (4, 1, 3, 0, 0),                               # one partly filled wave
    (5, 3, 3, 11, 2),                              # ragged last quad; later samples start off 16-byte alignment
    (64, 3, 0xDEADBEEFCAFEF00D, 5, 1),             # several blocks per sample, both key words in use
    (16, 4, 9, 2 ** 32 - 2, 0),                    # offset + k carries into hi32(s)
    (16, 2, 9, 2 ** 64 - 1, 4),                    # offset + k wraps
])
def test_single_layer_vs_reference(dev, res, n, seed, offset, layer):
    tab = Table([res], n + 1, dev)
    raw = tab.run(layer, seed, offset, n)
    check_against_reference(tab.images(raw, 0, n), seed, offset, layer, f"res {res}")


def test_three_layers_absolute_index_and_skipped_row(dev):
    """res 4 / (no noise_out) / 16 / 64 with first_layer = 5: the grid is sized by the largest layer, the small ones are partly filled
    blocks, and row i is layer 5 + i whether or not an earlier row is skipped."""
    tab = Table([4, None, 16, 64], 2, dev)
    raw = tab.run(5, 77, 1, 2)
    for i, layer in ((0, 5), (2, 7), (3, 8)):
        check_against_reference(tab.images(raw, i, 2), 77, 1, layer, f"row {i}")
    # a sub-range of the table (callers pass table + lo and first_layer = lo): same images, rows outside it untouched
    sub = tab.run(7, 77, 1, 2, rows=(2, 2))
    assert (sub[0] == CANARY).all()
    np.testing.assert_array_equal(sub[2], raw[2])
    np.testing.assert_array_equal(sub[3], raw[3])


def test_state_pointer_equals_by_value(dev):
    tab = Table([5, 32], 3, dev)
    seed, offset = 0x0123456789ABCDEF, 2 ** 64 - 2
    want = tab.run(0, seed, offset, 3)
    as_i64 = lambda v: v - 2 ** 64 if v >= 2 ** 63 else v
    state = torch.tensor([as_i64(seed), as_i64(offset)], dtype=torch.int64, device=dev)
    got = tab.run(0, 0x5555555555555555, 12345, 3, state=state)          # garbage by-value arguments are ignored
    for w, g in zip(want, got):
        np.testing.assert_array_equal(g, w)
    check_against_reference(tab.images(got, 1, 3), seed, offset, 1, "state")


def test_strength_is_one_fp32_multiply(dev):
    strength = [torch.tensor([0.37], dtype=torch.float32, device=dev), torch.tensor([-1.75], dtype=torch.float32, device=dev)]
    plain, scaled = Table([5, 32], 2, dev), Table([5, 32], 2, dev, strength=strength)
    a, b = plain.run(3, 21, 4, 2), scaled.run(3, 21, 4, 2)
    for i, s in enumerate((np.float32(0.37), np.float32(-1.75))):
        np.testing.assert_array_equal(scaled.images(b, i, 2), plain.images(a, i, 2) * s)


def test_batch_split_bit_for_bit(dev):
    tab = Table([5, 16, 64], 5, dev)
    whole = tab.run(0, 42, 7, 5)
    whole = [tab.images(whole, i, 5).copy() for i in range(3)]
    for k in range(5):
        one = tab.run(0, 42, 7 + k, 1)
        for i in range(3):
            np.testing.assert_array_equal(tab.images(one, i, 1)[0], whole[i][k], err_msg=f"row {i} sample {k}")


def test_seed_layer_and_offset_select_independent_streams(dev):
    """Independent streams are exact properties of the reference: every variant is checked against it, and differs from the base."""
    tab = Table([32], 1, dev)
    base = tab.images(tab.run(2, 5, 7, 1), 0, 1).copy()
    check_against_reference(base, 5, 7, 2, "base")
    for seed, offset, layer in ((6, 7, 2), (5 + 2 ** 32, 7, 2), (5, 8, 2), (5, 7 + 2 ** 32, 2), (5, 7, 3)):
        other = tab.images(tab.run(layer, seed, offset, 1), 0, 1)
        check_against_reference(other, seed, offset, layer, f"{(seed, offset, layer)}")
        assert (other != base).mean() > 0.9, (seed, offset, layer)


@pytest.mark.parametrize("seed", STAT_SEEDS)
def test_statistics(dev, seed):
    tab = Table([STAT_RES], STAT_N, dev)
    z = tab.images(tab.run(0, seed, 0, STAT_N), 0, STAT_N)
    assert z.size == 16384
    check_statistics(z, f"seed {seed}")


def test_refused_calls(dev):
    tab = Table([8], 1, dev)
    lib, t = _lib.lib(), tab.dev_table.data_ptr()
    for args in ((None, 0, 1, 8, 1, 0, None, 1), (t, 0, 0, 8, 1, 0, None, 1), (t, 0, 65536, 8, 1, 0, None, 1), (t, 0, 1, 0, 1, 0, None, 1),
                 (t, 0, 1, 8, 1, 0, None, 0), (t, 0, 1, 8, 1, 0, None, 65536), (t, -1, 1, 8, 1, 0, None, 1)):
        assert lib.nb_noise_seeded_f32(*args, stream()) == _lib.NB_EINVAL, args
    torch.cuda.synchronize()
    assert all((b.cpu().numpy() == CANARY).all() for b in tab.bufs)
