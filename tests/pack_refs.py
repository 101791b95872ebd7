"""The three activation operand formats of the split-f16 convolutions -- H2, "f8", "f6" -- restated on the host, bit for bit.
TEST INFRASTRUCTURE: no GPU, no library call; numpy, and for f6 the code table, rounding and field packing of ops (e2m3_encode,
f6_block_exponent, pack_f6_fields, F6_CH: tests/test_f6_format_cpu.py holds those to the table).  The definitions are the ones of
include/neube_hip.h and of the format comments of csrc/nb_h3_common.h, not a transcription of the packing kernels.
tests/test_pack_refs_cpu.py holds this file to those definitions; tests/test_hip_pack_formats.py holds the seven packing entry
points (nb_pack_h2_f32, nb_pack_h2f8_f32, nb_pack_h2f6_f32, their _part forms, nb_pack_h2_ranged_f32) to this file.

Container (all formats): uint16 [n, c8_total, 2 (hi, lo), hw, 8]; channel ch of the call lies in group cg0 + ch // 8, element ch % 8.
    v = float32(x) * float32(scale[n * scale_stride + ch])  -- ONE float32 multiply; v = x without a scale.  x = x1 ++ x2 along the
    channels; channels >= c1 + c2 of the last group are 0.
H2   slot (cg, hi) = f16(v), round to nearest even;  slot (cg, lo) = f16(v - float32(f16(v)))
f8   hi slots as H2.  Per 16-channel chunk k (groups 2k, 2k + 1), with xl = v - float32(f16(v)):
         the 16 bytes of slot (2k, lo)     = e4m3(clamp(xl * 512, +-448)) of the chunk's channels 0 .. 15, in channel order
         the 16 bytes of slot (2k + 1, lo) = e4m3(clamp(v * 0.25, +-448))
     e4m3 = OCP e4m3fn: 4 exponent bits (bias 7), 3 mantissa bits, subnormals (smallest 2^-9), round to nearest even, top 448 = 0x7E.
f6   hi slots as H2.  Per chunk: m = its largest |v|; scale byte = floor(log2 m) - 2 + 127 (0 for an all-zero chunk), S = 2^(byte - 127);
         field 2i = e2m3(xl[ch(i)] * 2048 / S), field 2i + 1 = e2m3(v[ch(i)] / S), ch(i) = channels 0-3, 8-11, 4-7, 12-15;
         the 32 fields are a little-endian 6-bit stream of 24 bytes: bytes 0 .. 15 = slot (2k, lo), bytes 16 .. 23 = the start of
         slot (2k + 1, lo), then the scale byte, then seven zero bytes.

DOMAIN in which this restatement claims to equal the device, bit for bit:
    - every input (and scale) is finite;
    - |v| < 65520: at and above it f16(v) is +-inf and the lo half -+inf (hi + lo = NaN) -- numpy and the device may well agree
      there too, but nothing is claimed;
    - f6: a chunk that is not all zero has m >= 2^-100 (below it the device's m * 0.25 leaves the normal float32 range that its
      exponent byte is read from, and ops.f6_block_exponent clamps).
Sign of a zero code (an fp8 or e2m3 code for -0.0, or for a negative magnitude that rounds to zero): the restatement keeps the
sign (0x80 / 0x20), as torch's e4m3 cast does.  tests/test_hip_pack_formats.py says in its header what the device does."""
import numpy as np
import torch

E4M3_MAX = 448.0


# ---------------------------------------------------------------------------------------------------------------------
# e4m3, in integer arithmetic on the float32 bit pattern (independent of torch's cast, which the CPU test compares it with)
# ---------------------------------------------------------------------------------------------------------------------

def e4m3_encode(x):
    """float32 array (finite) -> uint8 e4m3fn codes, round to nearest even, subnormals, magnitudes above 448 -> 0x7E (callers clamp)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    b = x.view(np.uint32).astype(np.int64)
    sign = (b >> 24) & 0x80
    a = b & 0x7FFFFFFF
    e = a >> 23                                         # biased float32 exponent: value = 1.m * 2^(e - 127)
    m = a & 0x7FFFFF
    # normal e4m3 (value >= 2^-6, e >= 121): exponent field e - 120, three mantissa bits; the 20 dropped bits round to nearest even and
    # a carry runs into the exponent by itself
    t = a - (120 << 23)
    code_n = t >> 20
    rem = t & 0xFFFFF
    code_n = code_n + ((rem > 0x80000) | ((rem == 0x80000) & ((code_n & 1) == 1)))
    # subnormal e4m3 (value < 2^-6): code = RNE(value * 2^9) = RNE(M * 2^(e - 141)), M = the 24-bit significand (7 -> 8 is the first normal)
    big = np.where(e > 0, m | 0x800000, 0)              # float32 subnormals (< 2^-126) round to zero
    sh = np.clip(141 - e, 1, 40)
    code_s = big >> sh
    rem_s = big & ((np.int64(1) << sh) - 1)
    half = np.int64(1) << (sh - 1)
    code_s = code_s + ((rem_s > half) | ((rem_s == half) & ((code_s & 1) == 1)))
    code = np.where(e >= 121, code_n, code_s)
    return (np.minimum(code, 0x7E) | sign).astype(np.uint8)


def _e4m3_table():
    t = np.empty(256, dtype=np.float64)
    for c in range(256):
        e, m = (c >> 3) & 15, c & 7
        v = m * 2.0 ** -9 if e == 0 else (1 + m / 8) * 2.0 ** (e - 7)
        t[c] = np.nan if (c & 0x7F) == 0x7F else (-v if c & 0x80 else v)
    return t


E4M3_VALUE = _e4m3_table()                              # code -> float64 (0x7F / 0xFF: NaN)


def e4m3_decode(codes):
    return E4M3_VALUE[np.asarray(codes, dtype=np.uint8)]


# ---------------------------------------------------------------------------------------------------------------------
# shared: v, its halves, the container
# ---------------------------------------------------------------------------------------------------------------------

def _f32(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32)


def values(x1, x2=None, scale=None, scale_stride=None):
    """v [n, c1 + c2, hw] float32 = (x1 ++ x2) * scale[n * scale_stride + ch] (scale: any shape, read flat from its first element, as
    the entry points read their pointer; scale_stride: c1 + c2 unless given)."""
    x = _f32(x1)
    x = x.reshape(x.shape[0], x.shape[1], -1)
    if x2 is not None and _f32(x2).shape[1] > 0:
        y = _f32(x2)
        x = np.concatenate([x, y.reshape(y.shape[0], y.shape[1], -1)], axis=1)
    if scale is None:
        return x
    n, c, _ = x.shape
    s = _f32(scale).reshape(-1)
    stride = c if scale_stride is None else scale_stride
    idx = np.arange(n)[:, None] * stride + np.arange(c)[None]
    return x * s[idx][:, :, None]                       # float32 x float32 -> one float32 multiply


def split(v):
    """(f16(v), float32(v - float32(f16(v))))"""
    with np.errstate(over="ignore", invalid="ignore"):
        hi = v.astype(np.float16)
        return hi, v - hi.astype(np.float32)


def _container(n, c, hw, c8_total, cg0, into, chunked):
    g = (c + 7) // 8
    if chunked:
        assert c % 16 == 0 and cg0 % 2 == 0, "f8 / f6: whole 16-channel chunks, an even first group"
    c8_total = cg0 + g if c8_total is None else c8_total
    assert cg0 >= 0 and cg0 + g <= c8_total
    if into is None:
        into = np.zeros([n, c8_total, 2, hw, 8], dtype=np.uint16)
    assert into.dtype == np.uint16 and into.shape == (n, c8_total, 2, hw, 8), (into.shape, (n, c8_total, 2, hw, 8))
    return into, g


def _grouped(a, g):
    """[n, c, hw] -> [n, g, hw, 8], zero channels behind c"""
    n, c, hw = a.shape
    p = np.zeros([n, g * 8, hw], dtype=a.dtype)
    p[:, :c] = a
    return p.reshape(n, g, 8, hw).transpose(0, 1, 3, 2)


def _bytes_to_words(b):
    """[..., 16] uint8 -> [..., 8] uint16, little endian"""
    b = b.astype(np.uint16)
    return b[..., 0::2] | (b[..., 1::2] << 8)


def _words_to_bytes(w):
    w = np.asarray(w, dtype=np.uint16)
    return np.stack([w & 0xFF, w >> 8], axis=-1).reshape(*w.shape[:-1], w.shape[-1] * 2).astype(np.uint8)


def _chunked(a):
    """[n, c, hw] -> [n, c / 16, hw, 16]: a chunk's channels, in channel order, per pixel"""
    n, c, hw = a.shape
    return a.reshape(n, c // 16, 16, hw).transpose(0, 1, 3, 2)


def _unchunked(a):
    n, k, hw, _ = a.shape
    return a.transpose(0, 1, 3, 2).reshape(n, k * 16, hw)


# ---------------------------------------------------------------------------------------------------------------------
# encoders
# ---------------------------------------------------------------------------------------------------------------------

def encode_h2(x1, x2=None, scale=None, scale_stride=None, c8_total=None, cg0=0, into=None):
    v = values(x1, x2, scale, scale_stride)
    n, c, hw = v.shape
    out, g = _container(n, c, hw, c8_total, cg0, into, False)
    hi, xl = split(v)
    with np.errstate(over="ignore", invalid="ignore"):
        lo = xl.astype(np.float16)
    out[:, cg0:cg0 + g, 0] = _grouped(hi.view(np.uint16), g)
    out[:, cg0:cg0 + g, 1] = _grouped(lo.view(np.uint16), g)
    return out


def encode_f8(x1, x2=None, scale=None, scale_stride=None, c8_total=None, cg0=0, into=None):
    v = values(x1, x2, scale, scale_stride)
    n, c, hw = v.shape
    out, g = _container(n, c, hw, c8_total, cg0, into, True)
    hi, xl = split(v)
    out[:, cg0:cg0 + g, 0] = _grouped(hi.view(np.uint16), g)
    clamp = lambda t: np.clip(t, np.float32(-E4M3_MAX), np.float32(E4M3_MAX))
    out[:, cg0:cg0 + g:2, 1] = _bytes_to_words(_chunked(e4m3_encode(clamp(xl * np.float32(512.0)))))
    out[:, cg0 + 1:cg0 + g:2, 1] = _bytes_to_words(_chunked(e4m3_encode(clamp(v * np.float32(0.25)))))
    return out


def f6_scale_byte(m):
    """float64 tensor of chunk maxima -> the E8M0 byte: floor(log2 m) - 2 + 127, 0 for an all-zero chunk"""
    from brushstroke_engine_amd import ops
    return torch.where(m > 0, ops.f6_block_exponent(m) + 127, torch.zeros_like(m)).to(torch.int64)


def encode_f6(x1, x2=None, scale=None, scale_stride=None, c8_total=None, cg0=0, into=None):
    from brushstroke_engine_amd import ops
    v = values(x1, x2, scale, scale_stride)
    n, c, hw = v.shape
    out, g = _container(n, c, hw, c8_total, cg0, into, True)
    hi, xl = split(v)
    out[:, cg0:cg0 + g, 0] = _grouped(hi.view(np.uint16), g)
    # the two field values as the float32 numbers the format names, then everything in float64: a division by a power of two is exact
    # there, so each field is rounded once
    a = torch.from_numpy(_chunked(xl * np.float32(2048.0))).double()          # [n, chunk, hw, 16]
    b = torch.from_numpy(_chunked(v)).double()
    byte = f6_scale_byte(b.abs().amax(dim=-1))                                # [n, chunk, hw]
    s = torch.exp2(byte.double() - 127.0)[..., None]
    fields = torch.stack([ops.e2m3_encode(a[..., ops.F6_CH] / s), ops.e2m3_encode(b[..., ops.F6_CH] / s)], dim=-1)
    by = ops.pack_f6_fields(fields.reshape(n, c // 16, hw, 32)).numpy()       # [n, chunk, hw, 24]
    second = np.zeros([n, c // 16, hw, 16], dtype=np.uint8)
    second[..., :8] = by[..., 16:]
    second[..., 8] = byte.numpy().astype(np.uint8)
    out[:, cg0:cg0 + g:2, 1] = _bytes_to_words(by[..., :16])
    out[:, cg0 + 1:cg0 + g:2, 1] = _bytes_to_words(second)
    return out


ENCODE = {"h2": encode_h2, "f8": encode_f8, "f6": encode_f6}


# ---------------------------------------------------------------------------------------------------------------------
# decoders: float64 planes [n, c, hw] of the first c channels from group cg0 on
# ---------------------------------------------------------------------------------------------------------------------

def _f16_plane(t, slot, c, cg0):
    g = (c + 7) // 8
    w = np.ascontiguousarray(t[:, cg0:cg0 + g, slot])                         # [n, g, hw, 8]
    n, _, hw, _ = w.shape
    return w.view(np.float16).astype(np.float64).transpose(0, 1, 3, 2).reshape(n, g * 8, hw)[:, :c]


def decode_h2(t, c, cg0=0):
    """(hi, lo)"""
    return _f16_plane(t, 0, c, cg0), _f16_plane(t, 1, c, cg0)


def decode_f8(t, c, cg0=0):
    """(hi, e4m3(xl * 512) decoded, e4m3(v / 4) decoded)"""
    assert c % 16 == 0 and cg0 % 2 == 0
    g = c // 8
    xl = e4m3_decode(_words_to_bytes(t[:, cg0:cg0 + g:2, 1]))                 # [n, chunk, hw, 16]
    xq = e4m3_decode(_words_to_bytes(t[:, cg0 + 1:cg0 + g:2, 1]))
    return _f16_plane(t, 0, c, cg0), _unchunked(xl), _unchunked(xq)


E2M3_VALUE = np.array([(m / 8 if e == 0 else (1 + m / 8) * 2.0 ** (e - 1)) * s for s in (1, -1) for e in range(4) for m in range(8)])


def f6_fields(t, c, cg0=0):
    """(codes [n, chunk, hw, 32], scale bytes [n, chunk, hw], the seven bytes behind the scale byte [n, chunk, hw, 7])"""
    assert c % 16 == 0 and cg0 % 2 == 0
    g = c // 8
    first = _words_to_bytes(t[:, cg0:cg0 + g:2, 1]).astype(np.int64)          # [n, chunk, hw, 16]
    second = _words_to_bytes(t[:, cg0 + 1:cg0 + g:2, 1]).astype(np.int64)
    by = np.concatenate([first, second[..., :8]], axis=-1)                    # the 24-byte stream
    bit = 6 * np.arange(32)
    lo_b, sh = bit // 8, bit % 8
    two = by[..., lo_b] | (by[..., np.minimum(lo_b + 1, 23)] << 8)            # (field 31 ends with byte 23: the clamped index is unused)
    return (two >> sh) & 63, second[..., 8], second[..., 9:]


def decode_f6(t, c, cg0=0):
    """(hi, the xl fields times S, the x fields times S, S [n, chunk, hw])"""
    codes, byte, _ = f6_fields(t, c, cg0)
    s = 2.0 ** (byte.astype(np.float64) - 127.0)
    val = E2M3_VALUE[codes] * s[..., None]                                    # field order
    ch = np.empty(16, dtype=np.int64)
    ch[[0, 1, 2, 3, 8, 9, 10, 11, 4, 5, 6, 7, 12, 13, 14, 15]] = np.arange(16)                  # channel -> field pair
    return _f16_plane(t, 0, c, cg0), _unchunked(val[..., 0::2][..., ch]), _unchunked(val[..., 1::2][..., ch]), s


# ---------------------------------------------------------------------------------------------------------------------
# inputs of tests/test_hip_pack_formats.py: the base distribution, the planted edge values (tests/test_pack_refs_cpu.py checks that they
# are what their comments say), and a report of where two containers differ
# ---------------------------------------------------------------------------------------------------------------------

def base_input(n, c, hw, seed):
    """randn x exp(randn per channel), float32 [n, c, hw]"""
    rs = np.random.RandomState(seed)
    return (rs.randn(n, c, hw) * np.exp(rs.randn(n, c, 1))).astype(np.float32)


EDGE_ALL = [
    0.0, -0.0,
    65504.0,                              # the largest f16
    65519.0,                              # the last float32 integer below the overflow threshold 65520: hi = 65504, lo = 15
    2.0 ** -14,                           # the smallest normal f16
    2.0 ** -24,                           # the smallest subnormal f16
    3 * 2.0 ** -25,                       # a tie between 2^-24 and 2^-23: hi = 2^-23, lo = -2^-25 -> a tie again, to zero
    2.0 ** -25,                           # ties to zero: hi = 0, and lo = f16(2^-25) = 0
    1 + 2.0 ** -11,                       # a tie for hi: to 1.0, lo = 2^-11
    1 + 2.0 ** -11 + 2.0 ** -23,          # just above it: hi = 1 + 2^-10, xl = -(2^-11 - 2^-23), a tie of lo: -2^-11
    1 + 2.0 ** -20,                       # lo = 2^-20: an f16 subnormal, exact
    0.125 + 3 * 2.0 ** -25,               # lo = 3 2^-25: a tie between the subnormals 2^-24 and 2^-23, to 2^-23
]
EDGE_F8 = [
    4.25, 4.75,                           # v / 4 = 1.0625, 1.1875: ties of e4m3 (step 0.125 at 1), to 1.0 and 1.25
    1792.0, 1800.0, 2000.0, 60000.0,      # v / 4 >= 448: the fp8(v / 4) plane saturates from 1792 on, the hi half stays exact (these are
                                          # f16 values: xl = 0);
    2049.0, 2051.0, 60015.0,              # ... and with it the fp8(xl 512) plane: xl = 1 (a tie of hi, to 2048), -1, 15 -> 512, -512, 7680
    2049.75,                              # xl = -0.25: -128, inside the range next to a saturated v / 4
    4 * 2.0 ** -9, 4 * 2.0 ** -10,        # v / 4 = the smallest e4m3 subnormal, and half of it (a tie, to zero)
    2.0 ** -18, 2.0 ** -19,               # likewise for xl 512 (hi = 0 for neither: both are f16 values, xl = 0) ...
    1 + 2.0 ** -18, 1 + 2.0 ** -19,       # ... so here: hi = 1, xl 512 = 2^-9 and 2^-10
]
F6_TIES = [7.0, 0.0625, 0.1875, 1.9375, -0.3125, 2.125, 3.875, -2.375, 4.25, 4.75, 6.75, -7.25, 0.0, -0.0, 1.0, -1.0]
F6_TOP = [7.6, -7.9, 4.0, 3.99] * 4      # S = 1: (7.5 S, 8 S) saturates


def signed(vals):
    return np.array([s * v for v in vals for s in (1.0, -1.0)], dtype=np.float32)


def plant(x, vals):
    """Write vals into x [n, c, hw] at fixed positions spread over samples, channels and pixels (the last pixels of the last block
    among them).  Positions may coincide in a tiny tensor: the later value stays."""
    n, c, hw = x.shape
    for k, v in enumerate(vals):
        x[k % n, (3 * k + 1) % c, (hw - 1 - 5 * k) % hw] = v
    return x


def plant_f6_chunks(x):
    """The f6 cases that are a property of a whole 16-channel chunk, in the last chunk of sample 0 at the first seven pixels
    (hw >= 7): all zero; all zero with one -0.0 (scale byte 0, the sign bit alone in that channel's x field); one non-zero channel; a maximum that is exactly a power of two (S = 1 and S = 2^-5); the top of the range;
    ties of the e2m3 grid in its three step sizes (0.125, 0.25, 0.5 at S = 1)."""
    n, c, hw = x.shape
    if hw < 7:
        return x
    rs = np.random.RandomState(99)
    k = c - 16
    x[0, k:, 0] = 0.0
    x[0, k:, 1] = 0.0
    x[0, k + 9, 1] = -3.3
    body = rs.uniform(-3.9, 3.9, 16).astype(np.float32)
    body[3] = -4.0
    x[0, k:, 2] = body
    x[0, k:, 3] = body * np.float32(2.0 ** -5)
    x[0, k:, 4] = F6_TOP
    x[0, k:, 5] = F6_TIES
    x[0, k:, 6] = 0.0
    x[0, k + 6, 6] = -0.0
    return x


def edge_input(fmt, n, c, hw, seed):
    x = plant(base_input(n, c, hw, seed), signed(EDGE_ALL + (EDGE_F8 if fmt == "f8" else [])))
    return plant_f6_chunks(x) if fmt == "f6" else x


def differences(fmt, got, want, limit=6):
    """(number of differing words, True if they differ ONLY in the sign bit of zero fp8 / e2m3 codes, a description)"""
    bad = np.argwhere(got != want)
    if not len(bad):
        return 0, False, "identical"
    lines = [f"[n {i[0]}, group {i[1]}, {'lo' if i[2] else 'hi'}, pixel {i[3]}, word {i[4]}] got 0x{got[tuple(i)]:04x} want 0x{want[tuple(i)]:04x}"
             for i in bad[:limit]]
    n_hi = int((bad[:, 2] == 0).sum())
    sign_only = False
    if fmt == "f8" and n_hi == 0:
        g, w = _words_to_bytes(got[:, :, 1]), _words_to_bytes(want[:, :, 1])
        d = g != w
        sign_only = bool(np.all((g[d] ^ w[d]) == 0x80) and np.all((w[d] & 0x7F) == 0))
    if fmt == "f6" and n_hi == 0 and got.shape[1] % 2 == 0:
        c = got.shape[1] * 8
        (g, gb, gp), (w, wb, wp) = f6_fields(got, c), f6_fields(want, c)
        d = g != w
        sign_only = bool(np.array_equal(gb, wb) and np.array_equal(gp, wp) and np.all((g[d] ^ w[d]) == 0x20) and np.all((w[d] & 0x1F) == 0))
    return len(bad), sign_only, (f"{len(bad)} of {got.size} words differ ({n_hi} in hi slots); only in the sign of zero codes: {sign_only}; first: "
                                 + "; ".join(lines))
