"""numpy restatement of the seeded-noise generator of include/neube_hip.h (nb_noise_seeded_f32): Philox4x32-10 on uint64 arrays
and the uniform / Box-Muller mapping in float64 from the same integers.  Helper of the seeded-noise tests; pinned on the CPU by
tests/test_seeded_noise_cpu.py (Random123 known answers)."""
import math

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF
MASK64 = (1 << 64) - 1


def philox4x32_10(counter, key):
    """counter: four, key: two broadcastable arrays (or ints) of 32-bit values -> four uint64 arrays holding 32-bit values."""
    c = [np.asarray(v, dtype=np.uint64) & np.uint64(MASK32) for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & MASK32, int(key[1]) & MASK32
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]                 # 32 x 32 -> 64 bits: exact in uint64
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & np.uint64(MASK32),
             (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & np.uint64(MASK32)]
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return c


def normal_pair(a, b):
    """Two arrays of 32-bit draws -> (z_even, z_odd, r) in float64: u1 = ((a >> 8) + 1) 2^-24 in (0, 1], u2 = (b >> 8) 2^-24 in
    [0, 1), r = sqrt(-2 ln u1), z = r (cos, sin)(2 pi u2)."""
    u1 = ((a >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24
    t = (b >> np.uint64(8)).astype(np.int64)                      # angle = pi t / 2^23; the quadrant is reduced exactly in integers
    r = np.sqrt(-2.0 * np.log(u1))
    quad, frac = t >> 22, (t & ((1 << 22) - 1)).astype(np.float64) * (np.pi / 2 ** 23)      # angle = quad pi/2 + frac, frac < pi/2
    cf, sf = np.cos(frac), np.sin(frac)
    cos = np.choose(quad, [cf, -sf, -cf, sf])
    sin = np.choose(quad, [sf, cf, -sf, -cf])
    return r * cos, r * sin, r


def seeded_noise(seed, offset, layer, k, res):
    """Sample k of layer `layer` (absolute index): (z64, r64), each [res, res] float64 -- the normals before the strength multiply and
    the Box-Muller radius of every pixel (the scale of the test's bound)."""
    npix = res * res
    quads = (npix + 3) // 4
    s = (int(offset) + int(k)) & MASK64
    seed = int(seed) & MASK64
    q = np.arange(quads, dtype=np.uint64)
    x = philox4x32_10((q, layer, s & MASK32, s >> 32), (seed & MASK32, seed >> 32))
    z0, z1, r01 = normal_pair(x[0], x[1])
    z2, z3, r23 = normal_pair(x[2], x[3])
    z = np.stack([z0, z1, z2, z3], axis=1).reshape(-1)[:npix].reshape(res, res)
    r = np.stack([r01, r01, r23, r23], axis=1).reshape(-1)[:npix].reshape(res, res)
    return z, r


# The seeds of the GPU statistics test (tests/test_hip_noise_seeded.py): fixed after
# tests/test_seeded_noise_cpu.py::test_reference_statistics_at_the_gpu_tests_seeds passed for each of them on the float64 restatement alone.
STAT_SEEDS = (1, 20261019, 0x9E3779B97F4A7C15)
STAT_RES, STAT_N = 64, 4


def stat_bounds(n_values):
    """(|mean|, |var - 1|, max |z|) bounds for N standard normals: five standard errors of the sample mean (1 / sqrt N) and of the sample
    variance (sqrt(2 / N)), and the largest radius the generator can produce at all, sqrt(-2 ln 2^-24) = sqrt(48 ln 2)."""
    return 5.0 / math.sqrt(n_values), 5.0 * math.sqrt(2.0 / n_values), math.sqrt(48.0 * math.log(2.0))


def check_statistics(z, what):
    z = np.asarray(z, dtype=np.float64).reshape(-1)
    m_max, v_max, z_max = stat_bounds(z.size)
    assert np.isfinite(z).all(), what
    assert abs(z.mean()) <= m_max, (what, z.mean())
    assert abs(z.var() - 1.0) <= v_max, (what, z.var())
    assert np.abs(z).max() <= z_max, (what, np.abs(z).max())
