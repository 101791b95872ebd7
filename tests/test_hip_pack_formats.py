"""GPU: the seven activation packers of the split-f16 convolutions, each through its C entry point, BIT FOR BIT against the host
restatement of the operand formats (tests/pack_refs.py, held to include/neube_hip.h without a GPU by tests/test_pack_refs_cpu.py):

    nb_pack_h2_f32, nb_pack_h2f8_f32, nb_pack_h2f6_f32                  csrc/nb_pack_h2.hip   x1 ++ x2, with and without a scale
    nb_pack_h2_part_f32, nb_pack_h2f8_part_f32, nb_pack_h2f6_part_f32   csrc/nb_pack_h2.hip   into groups cg0 .. of a wider tensor
    nb_pack_h2_ranged_f32                                               csrc/nb_grad.hip      the scale times the power of two k

All seven are pure conversions and the library is built without contraction, so no tolerance appears anywhere in this file: the whole
container is compared with encode(...) as integers.  Every output lies in a buffer pre-filled with the f16 NaN pattern 0x7E00 with
guard words on both sides; the guards, and for the _part calls every group outside [cg0, cg0 + ceil(c / 8)), must keep that pattern
(the _part reference is encode(..., into=<the fill>), so the comparison of the whole container says that too).

Shapes (n, c1, c2, h, w): one pixel; hw = 255 / 256 / 257 around the 256-thread block; hw = 1000 (four blocks, a ragged last one);
c1 % 8 != 0 so that x1 ++ x2 meets inside a group (and, f8 / f6, inside a chunk); c % 8 != 0 for H2 (zero channels).  _part calls:
the scale pointer starts 8 cg0 floats into a [n, scale_stride] styles row, as networks.py passes `styles + c_prod`.
Values: randn x exp(randn per channel); without a scale (v = the planted value) pack_refs.EDGE_ALL / EDGE_F8 and the f6 chunks of
pack_refs.plant_f6_chunks are planted at fixed positions, each with both signs.

Sign of zero codes: the comparison is strict -- the device writes the same sign bit as the restatement into fp8 and e2m3 codes whose
magnitude is zero (-0.0, negative values that round to zero), so the allowance "compare zero codes by value" is not used."""
import numpy as np
import pytest
import torch

import pack_refs as pr

pytestmark = pytest.mark.gpu

GUARD = 64                                            # words before and after every output (keeps 16-byte alignment)
FILL = 0x7E00                                         # an f16 NaN

FULL = {"h2": "nb_pack_h2_f32", "f8": "nb_pack_h2f8_f32", "f6": "nb_pack_h2f6_f32"}
PART = {"h2": "nb_pack_h2_part_f32", "f8": "nb_pack_h2f8_part_f32", "f6": "nb_pack_h2f6_part_f32"}

SHAPES_H2 = [(1, 1, 0, 1, 1), (3, 20, 5, 5, 51), (2, 7, 9, 16, 16), (1, 13, 0, 1, 257), (2, 8, 24, 25, 40)]
SHAPES_16 = [(1, 16, 0, 1, 1), (3, 13, 19, 5, 51), (2, 48, 0, 16, 16), (1, 32, 16, 1, 257), (2, 5, 27, 25, 40)]
FULL_CASES = [(f, s) for f in ("h2", "f8", "f6") for s in (SHAPES_H2 if f == "h2" else SHAPES_16)]
# (c, cg0, c8_total, scale_stride)
PARTS_H2 = [(5, 3, 6, 53), (24, 0, 3, 24)]
PARTS_16 = [(16, 2, 6, 48), (32, 4, 8, 80), (16, 0, 4, 32)]
PART_CASES = [(f, p) for f in ("h2", "f8", "f6") for p in (PARTS_H2 if f == "h2" else PARTS_16)]


class Out:
    """A container [n, c8_total, 2, hw, 8] of 16-bit words inside a buffer filled with FILL, GUARD words on either side."""

    def __init__(self, n, c8_total, hw):
        self.shape = (n, c8_total, 2, hw, 8)
        self.numel = int(np.prod(self.shape))
        self.buf = torch.full([self.numel + 2 * GUARD], FILL, dtype=torch.int16, device="cuda")
        self.ptr = self.buf.data_ptr() + 2 * GUARD
        assert self.ptr % 16 == 0

    def read(self):
        """(the container as uint16, True if both guards still hold the fill pattern)"""
        w = self.buf.cpu().numpy().view(np.uint16)
        guards = bool(np.all(w[:GUARD] == FILL) and np.all(w[-GUARD:] == FILL))
        return w[GUARD:GUARD + self.numel].reshape(self.shape).copy(), guards

    def untouched(self, mask):
        """The guards and the groups under `mask` [c8_total] still hold the fill pattern, bit for bit."""
        t, guards = self.read()
        return guards and bool(np.all(t[:, mask] == FILL))


def _lib():
    from brushstroke_engine_amd import _lib
    return _lib.lib()


def _check(rc, what):
    from brushstroke_engine_amd import _lib
    _lib.check(rc, what)


def P(t):
    return None if t is None else t.data_ptr()


def _scale(n, width, seed):
    """styles of both signs, 0.5 <= |s| < 1.5"""
    rs = np.random.RandomState(seed)
    return (rs.uniform(0.5, 1.5, (n, width)) * rs.choice([-1.0, 1.0], (n, width))).astype(np.float32)


def _same(fmt, out, want, what):
    got, guards = out.read()
    assert guards, f"{what}: a guard word was written"
    k, sign_only, text = pr.differences(fmt, got, want)
    print(f"[pack-formats] {what}: {got.size} words, {text}")
    assert k == 0, f"{what}: {text}"


def _run_full(fmt, shape, scaled, side_stream=False):
    n, c1, c2, h, w = shape
    c, hw = c1 + c2, h * w
    seed = 1000 * c + hw + scaled
    x = pr.base_input(n, c, hw, seed) if scaled else pr.edge_input(fmt, n, c, hw, seed)
    sc = _scale(n, c, seed + 1) if scaled else None
    # .copy(): the two halves as separate dense tensors, as the entry point takes them
    x1 = torch.from_numpy(x[:, :c1].copy()).cuda()
    x2 = torch.from_numpy(x[:, c1:].copy()).cuda() if c2 else None
    scd = None if sc is None else torch.from_numpy(sc).cuda()
    out = Out(n, (c + 7) // 8, hw)
    what = f"{FULL[fmt]} n {n} c {c1}+{c2} hw {hw}" + (" x scale" if scaled else " edges") + (" side stream" if side_stream else "")
    fn = getattr(_lib(), FULL[fmt])
    if side_stream:
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        _check(fn(P(x1), c1, P(x2), c2, P(scd), out.ptr, n, hw, s.cuda_stream), what)
        s.synchronize()
    else:
        _check(fn(P(x1), c1, P(x2), c2, P(scd), out.ptr, n, hw, torch.cuda.current_stream().cuda_stream), what)
        torch.cuda.synchronize()
    want = pr.ENCODE[fmt](x[:, :c1], x[:, c1:] if c2 else None, scale=sc)
    _same(fmt, out, want, what)


@pytest.mark.parametrize("scaled", [False, True], ids=["edges", "scaled"])
@pytest.mark.parametrize("fmt,shape", FULL_CASES, ids=lambda v: v if isinstance(v, str) else "n{}_c{}+{}_{}x{}".format(*v))
def test_full_packers_bit_for_bit(fmt, shape, scaled):
    """nb_pack_h2_f32 / nb_pack_h2f8_f32 / nb_pack_h2f6_f32 == encode(x1, x2, scale): every word of the container, guards intact."""
    _run_full(fmt, shape, scaled)


@pytest.mark.parametrize("fmt", ["h2", "f8", "f6"])
def test_full_packers_on_a_side_stream(fmt):
    """The same on a non-default stream ordered behind the current one, followed by a synchronise of that stream (the generator's
    pack_stream)."""
    _run_full(fmt, SHAPES_H2[1] if fmt == "h2" else SHAPES_16[1], True, side_stream=True)


@pytest.mark.parametrize("scaled", [True, False], ids=["scaled", "edges"])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("hw", [255, 257])
@pytest.mark.parametrize("fmt,part", PART_CASES, ids=lambda v: v if isinstance(v, str) else "c{}_cg{}_of{}_stride{}".format(*v))
def test_part_packers_bit_for_bit(fmt, part, hw, n, scaled):
    """nb_pack_h2*_part_f32 == encode(x, scale = styles + 8 cg0, scale_stride, c8_total, cg0, into = the fill): the groups of the call
    bit for bit, every other group and the guards still the fill pattern."""
    c, cg0, c8_total, stride = part
    seed = 7000 + 100 * c + 10 * cg0 + hw + n
    x = pr.base_input(n, c, hw, seed) if scaled else pr.edge_input(fmt, n, c, hw, seed)
    styles = _scale(n, stride, seed + 1)
    off = 8 * cg0
    assert off + c <= stride
    xd, std = torch.from_numpy(x).cuda(), torch.from_numpy(styles).cuda()
    out = Out(n, c8_total, hw)
    what = f"{PART[fmt]} n {n} c {c} hw {hw} groups {cg0}.. of {c8_total}, stride {stride}" + (" x scale" if scaled else " edges")
    _check(getattr(_lib(), PART[fmt])(P(xd), c, std.data_ptr() + 4 * off if scaled else None, stride, out.ptr, c8_total, cg0, n, hw,
                                      torch.cuda.current_stream().cuda_stream), what)
    torch.cuda.synchronize()
    outside = np.ones(c8_total, dtype=bool)
    outside[cg0:cg0 + (c + 7) // 8] = False
    assert out.untouched(outside), f"{what}: a group outside {cg0} .. {cg0 + (c + 7) // 8 - 1}, or a guard, was written"
    fill = np.full(out.shape, FILL, dtype=np.uint16)
    want = pr.ENCODE[fmt](x, scale=styles.reshape(-1)[off:] if scaled else None, scale_stride=stride, c8_total=c8_total, cg0=cg0, into=fill)
    assert np.all(want[:, outside] == FILL) and not np.any(np.all(want[:, ~outside] == FILL, axis=(0, 2, 3, 4)))
    _same(fmt, out, want, what)


def test_ranged_packer_equals_the_shared_restatement():
    """nb_absmax_f32 + nb_pack_h2_ranged_f32 at (3, 21, 0, 9, 40) == encode_h2(x, scale * k), k = dco_in / dco_out read back (one power
    of two): the restatement of this file and h2_emulated of tests/test_hip_train_kernels.py say the same thing."""
    lib = _lib()
    n, c, h, w = 3, 21, 9, 40
    hw = h * w
    x = (pr.base_input(n, c, hw, 5) * np.float32(3e-5)).astype(np.float32)
    sc = _scale(n, c, 6)
    xd, scd = torch.from_numpy(x).cuda(), torch.from_numpy(sc).cuda()
    S = torch.cuda.current_stream().cuda_stream
    slots = torch.zeros([4], dtype=torch.int32, device="cuda")
    _check(lib.nb_absmax_f32(P(xd), xd.numel(), None, 0, P(scd), scd.numel(), P(slots), S), "absmax")
    dco_in = torch.from_numpy(np.random.RandomState(7).uniform(0.25, 1.25, (n, 50)).astype(np.float32)).cuda()
    dco_buf = torch.full([dco_in.numel() + 2 * GUARD], float("nan"), device="cuda")
    dco = dco_buf[GUARD:GUARD + dco_in.numel()]
    out = Out(n, (c + 7) // 8, hw)
    _check(lib.nb_pack_h2_ranged_f32(P(xd), c, None, 0, P(scd), out.ptr, n, hw, P(slots), 16384.0, P(dco_in), P(dco), dco_in.numel(), S),
           "pack_h2_ranged")
    torch.cuda.synchronize()
    assert bool(torch.isnan(dco_buf[:GUARD]).all() and torch.isnan(dco_buf[-GUARD:]).all()), "a guard of dco_out was written"
    k = (dco_in / dco.view(n, 50)).cpu().numpy().astype(np.float64)
    kk = float(k.flat[0])
    assert np.all(k == kk) and np.log2(kk) == np.round(np.log2(kk)), "dco_in / dco_out is not one power of two"
    m = float(np.abs(x).max()) * float(np.abs(sc).max())
    assert 2.0 ** 12 < m * kk <= 2.0 ** 14, f"range scale {kk} puts the maximum at {m * kk}"
    want = pr.encode_h2(x, scale=sc * np.float32(kk))                        # scale * k is exact: k is a power of two
    _same("h2", out, want, f"nb_pack_h2_ranged_f32 n {n} c {c} hw {hw}, k = 2^{int(np.log2(kk))}")
