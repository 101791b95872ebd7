"""No GPU: tests/pack_refs.py -- the host restatement of the H2 / "f8" / "f6" activation formats that tests/test_hip_pack_formats.py
holds the packing kernels to -- held to the formats' definitions (include/neube_hip.h): the e4m3 conversion code by code and against
torch's cast, the H2 halves, the f8 and f6 layouts through decoders that do not share the encoders' code paths, the f6 scale-byte rule
against the float32 exponent, and the `into` / cg0 semantics of the _part entry points."""
import numpy as np
import pytest
import torch

import pack_refs as pr


def _rand(shape, seed, spread=1.0):
    rs = np.random.RandomState(seed)
    return (rs.randn(*shape) * np.exp(spread * rs.randn(shape[0], shape[1], 1))).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# e4m3
# ---------------------------------------------------------------------------------------------------------------------

FINITE = np.array([c for c in range(256) if (c & 0x7F) != 0x7F], dtype=np.uint8)


def test_e4m3_table_is_the_format():
    v = pr.E4M3_VALUE
    assert v[0x7E] == 448.0 and v[0xFE] == -448.0 and v[0x01] == 2.0 ** -9 and v[0x08] == 2.0 ** -6 and v[0x38] == 1.0
    assert np.isnan(v[0x7F]) and np.isnan(v[0xFF]) and len(FINITE) == 254
    assert np.all(np.diff(v[:0x7F]) > 0)
    t = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).double().numpy()
    assert np.array_equal(t[FINITE], v[FINITE])


def test_e4m3_roundtrip_all_finite_codes():
    got = pr.e4m3_encode(pr.E4M3_VALUE[FINITE].astype(np.float32))
    assert np.array_equal(got, FINITE)                                       # -0.0 -> 0x80 included


def test_e4m3_midpoints_go_to_even_and_neighbours_to_nearest():
    v = pr.E4M3_VALUE[:0x7F]                                                 # 0 .. 448, ascending
    lo, hi = np.arange(0x7E), np.arange(1, 0x7F)
    mid = ((v[lo] + v[hi]) / 2).astype(np.float32)
    assert np.array_equal(mid.astype(np.float64), (v[lo] + v[hi]) / 2)       # every midpoint is a float32
    even = np.where(lo % 2 == 0, lo, hi).astype(np.uint8)
    for sign, bit in ((1.0, 0), (-1.0, 0x80)):
        s = np.float32(sign)
        assert np.array_equal(pr.e4m3_encode(s * mid), even | bit)
        below = np.nextafter(mid, np.float32(0))
        above = np.nextafter(mid, np.float32(np.inf))
        assert np.array_equal(pr.e4m3_encode(s * below), lo.astype(np.uint8) | bit)
        assert np.array_equal(pr.e4m3_encode(s * above), hi.astype(np.uint8) | bit)


def test_e4m3_saturation_after_the_clamp():
    big = np.array([448.0, np.nextafter(np.float32(448), np.float32(np.inf)), 449.0, 464.0, 480.0, 512.0, 1792.0, 65504.0, 3e38], dtype=np.float32)
    for s, code in ((1, 0x7E), (-1, 0xFE)):
        x = np.float32(s) * big
        assert np.all(pr.e4m3_encode(np.clip(x, -448, 448)) == code)
        assert np.all(pr.e4m3_encode(x) == code)                            # the conversion saturates by itself too
    assert pr.e4m3_encode(np.array([np.nextafter(np.float32(448), np.float32(0))], dtype=np.float32))[0] == 0x7E
    assert pr.e4m3_encode(np.array([432.0], dtype=np.float32))[0] == 0x7E   # the tie between 416 (0x7D) and 448: to the even code
    assert pr.e4m3_encode(np.array([431.9], dtype=np.float32))[0] == 0x7D


def test_e4m3_small_magnitudes_keep_the_sign_of_zero():
    tiny = np.array([0.0, 2.0 ** -10, 2.0 ** -11, 1e-10, 2.0 ** -126, 1e-40, 1e-45], dtype=np.float32)
    assert np.all(pr.e4m3_encode(tiny) == 0x00)
    assert np.all(pr.e4m3_encode(-tiny) == 0x80)
    up = np.nextafter(np.float32(2.0 ** -10), np.float32(1))
    assert pr.e4m3_encode(np.array([up, -up], dtype=np.float32)).tolist() == [0x01, 0x81]


def test_e4m3_equals_torch_cast_on_random_floats():
    rs = np.random.RandomState(11)
    n = 1 << 20
    # every binade from 2^-14 to 2^11 (both tails beyond the format), plus raw bit patterns restricted to finite values
    x = (rs.uniform(1, 2, n) * 2.0 ** rs.randint(-14, 12, n) * rs.choice([-1, 1], n)).astype(np.float32)
    bits = rs.randint(0, 1 << 32, n // 4, dtype=np.uint64).astype(np.uint32).view(np.float32)
    x[:n // 4] = np.where(np.isfinite(bits), bits, np.float32(1.5))
    want = torch.from_numpy(x).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    got = pr.e4m3_encode(np.clip(x, np.float32(-448), np.float32(448)))
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {n} differ"


# ---------------------------------------------------------------------------------------------------------------------
# H2
# ---------------------------------------------------------------------------------------------------------------------

def test_h2_halves_reproduce_v_and_pad_with_zeros():
    n, c, hw = 2, 21, 77
    x = _rand((n, c, hw), 1)
    sc = np.random.RandomState(2).uniform(-1.5, 1.5, (n, c)).astype(np.float32)
    t = pr.encode_h2(x, scale=sc)
    assert t.shape == (n, 3, 2, hw, 8) and t.dtype == np.uint16
    v = (x * sc[:, :, None]).astype(np.float32).astype(np.float64)
    hi, lo = pr.decode_h2(t, c)
    assert np.array_equal(hi, v.astype(np.float16).astype(np.float64))
    assert np.all(np.abs(hi + lo - v) <= 2.0 ** -25 + 2.0 ** -22 * np.abs(v))
    assert not t[:, 2, :, :, 5:].any()                                       # channels 21 .. 23
    full_hi, _ = pr.decode_h2(t, 24)
    assert np.array_equal(full_hi[:, :21], hi)


def test_h2_concatenation_lands_like_one_tensor():
    n, c1, c2, hw = 2, 13, 6, 40
    x = _rand((n, c1 + c2, hw), 3)
    sc = np.random.RandomState(4).uniform(0.5, 1.5, (n, c1 + c2)).astype(np.float32)
    for s in (None, sc):
        one = pr.encode_h2(x, scale=s)
        two = pr.encode_h2(x[:, :c1], x[:, c1:], scale=s)
        assert np.array_equal(one, two)
    for name in ("f8", "f6"):
        y = _rand((n, 32, hw), 5)
        assert np.array_equal(pr.ENCODE[name](y, scale=None), pr.ENCODE[name](y[:, :13], y[:, 13:]))


def test_values_is_one_float32_multiply_with_a_strided_scale():
    n, c, hw, stride, off = 3, 5, 9, 53, 24
    x = _rand((n, c, hw), 6)
    styles = np.random.RandomState(7).uniform(-2, 2, (n, stride)).astype(np.float32)
    v = pr.values(x, scale=styles.reshape(-1)[off:], scale_stride=stride)
    assert v.dtype == np.float32
    assert np.array_equal(v, x * styles[:, off:off + c, None])
    assert np.array_equal(pr.values(x.reshape(n, c, 3, 3)), x)


# ---------------------------------------------------------------------------------------------------------------------
# f8
# ---------------------------------------------------------------------------------------------------------------------

def test_f8_decoder_inverts_the_layout():
    """Channel j of chunk k holds its own exactly representable value: v / 4 = an e4m3 value, xl * 512 = another."""
    n, c, hw = 2, 48, 3
    q = pr.E4M3_VALUE[0x40 + np.arange(c)]                                   # 2 .. 120: 48 distinct codes, v / 4 = q
    l = pr.E4M3_VALUE[0x08 + np.arange(c)] * 2.0 ** -9                       # distinct, 2^-18 of 4 q: below half an f16 step, inside float32
    hi = (4 * q)[None, :, None] * np.array([1.0, -1.0])[:, None, None] * np.ones([1, 1, hw])
    lo = l[None, :, None] * np.array([1.0, 2.0, -1.0])[None, None, :] * np.ones([n, 1, 1])
    x = (hi + lo).astype(np.float32)
    assert np.array_equal(x.astype(np.float64), hi + lo)
    assert np.array_equal(x.astype(np.float16).astype(np.float64), hi)       # lo is below half an f16 step: hi survives
    t = pr.encode_f8(x)
    assert t.shape == (n, 6, 2, hw, 8)
    d_hi, d_xl, d_q = pr.decode_f8(t, c)
    assert np.array_equal(d_hi, hi)
    assert np.array_equal(d_xl, lo * 512)                                    # e4m3 values times a power of two: exact codes
    # v / 4 = q + lo / 4: lo / 4 is far below half an e4m3 step of q, so the plane is q with the sample's sign
    assert np.array_equal(d_q, hi / 4)


def test_f8_decoder_agrees_with_the_encoder_routes_decoder():
    import enc_refs as er
    n, c, h, w = 2, 32, 3, 5
    x = _rand((n, c, h * w), 8, spread=2.0)
    t = pr.encode_f8(x)
    hi, xl, q = pr.decode_f8(t, c)
    tt = torch.from_numpy(t.view(np.float16)).reshape(n, c // 8, 2, h, w, 8)
    v, plane, mask = er.decode_f8(tt, 0, c)
    assert np.array_equal(v.reshape(n, c, -1).numpy(), hi + xl / 512)
    assert np.array_equal(plane.reshape(n, c, -1).numpy(), q * 4)
    assert not bool(mask.any())


def test_f8_planes_are_the_definition():
    n, c, hw = 1, 16, 64
    x = _rand((n, c, hw), 9, spread=3.0)
    x[0, 0, :4] = [1792.0, -2000.0, 60000.0, 4.25]
    t = pr.encode_f8(x)
    v = torch.from_numpy(x)
    hi = v.half()
    f8 = lambda a: a.clamp(-448, 448).to(torch.float8_e4m3fn).double().numpy()
    d_hi, d_xl, d_q = pr.decode_f8(t, c)
    assert np.array_equal(d_hi, hi.double().numpy())
    assert np.array_equal(d_xl, f8((v - hi.float()) * 512.0))
    assert np.array_equal(d_q, f8(v * 0.25))
    assert d_q[0, 0, :4].tolist() == [448.0, -448.0, 448.0, 1.0]              # 4.25 / 4 = 1.0625: the tie goes to 1.0


# ---------------------------------------------------------------------------------------------------------------------
# f6
# ---------------------------------------------------------------------------------------------------------------------

def test_f6_fields_decode_like_ops_unpack():
    from brushstroke_engine_amd import ops
    n, c, h, w = 2, 48, 2, 7
    x = _rand((n, c, h * w), 10, spread=1.5)
    sc = np.random.RandomState(12).uniform(0.5, 1.5, (n, c)).astype(np.float32)
    t = pr.encode_f6(x, scale=sc)
    hi, xl, xv, s = pr.decode_f6(t, c)
    tt = torch.from_numpy(t.view(np.float16)).reshape(n, c // 8, 2, h, w, 8)
    o_hi, o_xl, o_xv, o_s = ops.unpack_h2f6(tt, c)
    assert np.array_equal(o_hi.reshape(n, c, -1).double().numpy(), hi)
    assert np.array_equal(o_xl.reshape(n, c, -1).double().numpy(), xl)
    assert np.array_equal(o_xv.reshape(n, c, -1).double().numpy(), xv)
    assert np.array_equal(o_s.reshape(n, c // 16, -1).double().numpy(), s)
    # and the fields stand for the values: x within half a step (S / 2 at the top of the range; (7.5 S, 8 S) saturates: one step)
    v = (x * sc[:, :, None]).astype(np.float32).astype(np.float64)
    srep = np.repeat(s, 16, axis=1)
    assert np.all(np.abs(xv - v) <= 0.5 * srep)
    _, byte, pad = pr.f6_fields(t, c)
    assert not pad.any()


def test_f6_scale_byte_rule():
    """byte = the float32 exponent field of m, minus 2 (frexp restates floor(log2 m) without a logarithm): at powers of two, just below
    them, and so that m / S lands in [4, 8)."""
    ms = []
    for k in (-100, -60, -14, -1, 0, 1, 2, 3, 10, 15):
        p = np.float32(2.0 ** k)
        ms += [p, np.nextafter(p, np.float32(0)), np.nextafter(p, np.float32(np.inf)), p * np.float32(1.5)]
    ms += [np.float32(65504.0), np.float32(65519.0), np.float32(7.5), np.float32(7.9999995)]
    m = np.array([v for v in ms if v >= np.float32(2.0 ** -100)], dtype=np.float32)
    x = np.zeros([1, 16, len(m)], dtype=np.float32)
    x[0, 5] = -m                                                             # a single non-zero channel, negative
    _, byte, _ = pr.f6_fields(pr.encode_f6(x), 16)
    _, ex = np.frexp(m.astype(np.float64))                                   # m = f 2^ex, f in [0.5, 1): floor(log2 m) = ex - 1
    assert np.array_equal(byte[0, 0], ex - 1 - 2 + 127)
    s = 2.0 ** (byte[0, 0] - 127.0)
    assert np.all((m / s >= 4) & (m / s < 8))
    hi, xl, xv, _ = pr.decode_f6(pr.encode_f6(x), 16)
    top = np.minimum(m.astype(np.float64) / s, 7.5)
    assert np.all(np.abs(-xv[0, 5] / s - top) <= 0.25)                        # the maximum itself: a code in [4, 7.5]


def test_f6_all_zero_chunk_is_32_zero_bytes():
    x = _rand((2, 32, 5), 13)
    x[1, 16:, 2] = 0.0
    t = pr.encode_f6(x)
    assert not t[1, 2:4, :, 2].any()                                         # hi slots too
    assert t[1, 2:4, 1, 1].any() and t[0, 2:4, 1, 2].any()
    codes, byte, pad = pr.f6_fields(t, 32)
    assert byte[1, 1, 2] == 0 and not codes[1, 1, 2].any() and (np.delete(byte.reshape(-1), 1 * 10 + 1 * 5 + 2) > 0).all()


def test_f6_saturation_and_ties():
    x = np.zeros([1, 16, 2], dtype=np.float32)
    x[0, :, 0] = [7.6, -7.9, 4.0, 3.99] * 4                                  # S = 1: (7.5, 8) saturates
    x[0, :, 1] = [7.0, 0.0625, 0.1875, 1.9375, -0.3125, 2.125, 3.875, -2.375, 4.25, 4.75, 6.75, -7.25, 0.0, -0.0, 1.0, -1.0]
    _, _, xv, s = pr.decode_f6(pr.encode_f6(x), 16)
    assert s[0, 0].tolist() == [1.0, 1.0]
    assert xv[0, :, 0].tolist() == [7.5, -7.5, 4.0, 4.0] * 4
    assert xv[0, :, 1].tolist() == [7.0, 0.0, 0.25, 2.0, -0.25, 2.0, 4.0, -2.5, 4.0, 5.0, 7.0, -7.0, 0.0, 0.0, 1.0, -1.0]


# ---------------------------------------------------------------------------------------------------------------------
# _part semantics
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,c,cg0,c8_total", [("h2", 5, 3, 6), ("h2", 24, 0, 3), ("f8", 16, 2, 6), ("f6", 32, 4, 8), ("f6", 16, 0, 4)])
def test_into_overwrites_only_its_groups(name, c, cg0, c8_total):
    n, hw = 3, 19
    enc = pr.ENCODE[name]
    g = (c + 7) // 8
    first = 8 * cg0
    x_all = _rand((n, first + c, hw), 14)
    stride = 8 * c8_total + 5
    styles = np.random.RandomState(15).uniform(0.5, 1.5, (n, stride)).astype(np.float32)
    fill = np.full([n, c8_total, 2, hw, 8], 0x7E00, dtype=np.uint16)
    got = enc(x_all[:, first:], scale=styles.reshape(-1)[first:], scale_stride=stride, c8_total=c8_total, cg0=cg0, into=fill.copy())
    inside = np.zeros(c8_total, dtype=bool)
    inside[cg0:cg0 + g] = True
    assert np.all(got[:, ~inside] == 0x7E00)
    assert not np.any(np.all(got[:, inside] == 0x7E00, axis=(0, 2, 3, 4)))   # every group of the range was written
    # ... and equals those groups of the encode of the concatenation
    if first:
        whole = enc(x_all[:, :first], x_all[:, first:], scale=styles, scale_stride=stride)
        assert np.array_equal(got[:, inside], whole[:, cg0:cg0 + g])
        # two parts make the whole
        both = enc(x_all[:, :first], scale=styles, scale_stride=stride, c8_total=c8_total, cg0=0, into=got)
        assert both is got and np.array_equal(both[:, :cg0 + g], whole) and np.all(both[:, cg0 + g:] == 0x7E00)
    else:
        assert np.array_equal(got[:, inside], enc(x_all, scale=styles, scale_stride=stride))


# ---------------------------------------------------------------------------------------------------------------------
# the planted edge values of tests/test_hip_pack_formats.py are what their comments say
# ---------------------------------------------------------------------------------------------------------------------

def _one(fmt, v):
    x = np.zeros([1, 16, 1], dtype=np.float32)
    x[0, 0, 0] = v
    return pr.ENCODE[fmt](x)


def test_edge_values_common():
    f16 = lambda w: float(np.array([w], dtype=np.uint16).view(np.float16)[0])
    halves = lambda v: tuple(f16(_one("h2", v)[0, 0, s, 0, 0]) for s in (0, 1))
    assert all(abs(v) < 65520 for v in pr.EDGE_ALL + pr.EDGE_F8)            # inside the domain
    assert halves(65504.0) == (65504.0, 0.0) and halves(-65519.0) == (-65504.0, -15.0)
    assert halves(2.0 ** -14) == (2.0 ** -14, 0.0) and halves(2.0 ** -24) == (2.0 ** -24, 0.0)
    assert halves(3 * 2.0 ** -25) == (2.0 ** -23, 0.0) and _one("h2", 3 * 2.0 ** -25)[0, 0, 1, 0, 0] == 0x8000      # lo = -2^-25 -> -0.0
    assert halves(2.0 ** -25) == (0.0, 0.0) and _one("h2", -2.0 ** -25)[0, 0, 0, 0, 0] == 0x8000
    assert _one("h2", -0.0)[0, 0, 0, 0, 0] == 0x8000 and _one("h2", -0.0)[0, 0, 1, 0, 0] == 0x0000                  # -0.0 - (-0.0) = +0.0
    assert halves(1 + 2.0 ** -11) == (1.0, 2.0 ** -11)
    assert halves(1 + 2.0 ** -11 + 2.0 ** -23) == (1 + 2.0 ** -10, -(2.0 ** -11))      # xl = -(2^-11 - 2^-23): a tie of lo
    assert halves(1 + 2.0 ** -20) == (1.0, 2.0 ** -20) and 2.0 ** -20 < 2.0 ** -14
    assert halves(0.125 + 3 * 2.0 ** -25) == (0.125, 2.0 ** -23)


def test_edge_values_f8():
    def planes(v):
        _, xl, q = pr.decode_f8(_one("f8", v), 16)
        return xl[0, 0, 0], q[0, 0, 0]
    assert planes(4.25)[1] == 1.0 and planes(4.75)[1] == 1.25 and planes(-4.75)[1] == -1.25
    for v in (1792.0, 1800.0, 2000.0, 60000.0):
        assert planes(v) == (0.0, 448.0) and planes(-v)[1] == -448.0
    assert planes(1791.0)[1] == 448.0 and planes(1663.0)[1] == 416.0       # (1664 is the tie between 416 and 448)
    assert planes(2049.0) == (448.0, 448.0) and planes(2051.0) == (-448.0, 448.0) and planes(60015.0) == (448.0, 448.0)
    assert planes(2049.75) == (-128.0, 448.0)
    assert planes(4 * 2.0 ** -9)[1] == 2.0 ** -9 and planes(4 * 2.0 ** -10)[1] == 0.0
    assert planes(1 + 2.0 ** -18)[0] == 2.0 ** -9 and planes(1 + 2.0 ** -19)[0] == 0.0
    # zero codes that carry a sign in this restatement
    lo_bytes = lambda v: pr._words_to_bytes(_one("f8", v)[0, :2, 1, 0])[:, 0].tolist()
    assert lo_bytes(-0.0) == [0x00, 0x80] and lo_bytes(-4 * 2.0 ** -10) == [0x00, 0x80] and lo_bytes(3 * 2.0 ** -25) == [0x80, 0x00]


def test_edge_chunks_f6():
    x = pr.plant_f6_chunks(pr.base_input(2, 32, 9, 0))
    t = pr.encode_f6(x)
    codes, byte, pad = pr.f6_fields(t, 32)
    _, xl, xv, s = pr.decode_f6(t, 32)
    assert byte[0, 1, 0] == 0 and not codes[0, 1, 0].any()
    assert np.count_nonzero(xv[0, 16:, 1]) == 1 and xv[0, 25, 1] == -3.25 and s[0, 1, 1] == 0.5
    assert s[0, 1, 2] == 1.0 and xv[0, 19, 2] == -4.0 and s[0, 1, 3] == 2.0 ** -5 and xv[0, 19, 3] == -4.0 * 2.0 ** -5
    assert xv[0, 16:, 4].tolist() == [7.5, -7.5, 4.0, 4.0] * 4
    assert xv[0, 16:, 5].tolist() == [7.0, 0.0, 0.25, 2.0, -0.25, 2.0, 4.0, -2.5, 4.0, 5.0, 7.0, -7.0, 0.0, 0.0, 1.0, -1.0]
    assert byte[0, 1, 6] == 0 and codes[0, 1, 6].tolist() == [0] * 21 + [0x20] + [0] * 10      # channel 6 = field pair 10: its x field
    assert t[0, 2, 0, 6, 6] == 0x8000 and np.count_nonzero(t[0, 2:4, 0, 6]) == 1
    assert np.array_equal(x[1], pr.base_input(2, 32, 9, 0)[1]) and np.array_equal(x[0, :16], pr.base_input(2, 32, 9, 0)[0, :16])
    assert pr.plant_f6_chunks(pr.base_input(1, 16, 1, 0)).any()              # too few pixels: left alone


def test_differences_reports_the_sign_of_zero_case():
    x = pr.edge_input("f8", 2, 32, 40, 1)
    want = pr.encode_f8(x)
    assert pr.differences("f8", want.copy(), want)[0] == 0
    got = want.copy()
    b = pr._words_to_bytes(got[:, :, 1])
    assert (b == 0x80).any()
    b[b == 0x80] = 0
    got[:, :, 1] = pr._bytes_to_words(b)
    k, sign_only, text = pr.differences("f8", got, want)
    assert k > 0 and sign_only, text
    got[0, 0, 1, 3, 2] ^= 0x0100
    assert not pr.differences("f8", got, want)[1]
    x6 = pr.edge_input("f6", 2, 32, 40, 1)
    want = pr.encode_f6(x6)
    codes, _, _ = pr.f6_fields(want, 32)
    assert (codes == 0x20).any()
    got = pr.encode_f6(np.where(x6 == 0, np.float32(0), x6))                # -0.0 -> +0.0: some sign-of-zero codes go
    got[:, :, 0] = want[:, :, 0]
    k, sign_only, text = pr.differences("f6", got, want)
    assert k > 0 and sign_only, text
    got[0, 1, 1, 7, 0] ^= 0x0001
    assert not pr.differences("f6", got, want)[1]
