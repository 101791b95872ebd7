// The counter-based generator of the seeded draws (nb_noise_seeded_f32, nb_synth_spline_*): Philox4x32-10 and the Box-Muller pair,
// shared by csrc/nb_noise_seeded.hip and csrc/nb_drawings.hip.  include/neube_hip.h states the generator; tests/philox_ref.py restates
// it in numpy.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#define NB_PHILOX_M0 0xD2511F53u
#define NB_PHILOX_M1 0xCD9E8D57u
#define NB_PHILOX_W0 0x9E3779B9u
#define NB_PHILOX_W1 0xBB67AE85u

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123 known answers are in
// tests/test_seeded_noise_cpu.py): ten rounds, the key bumped between them.
__host__ __device__ __forceinline__ void nb_philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                                          uint32_t out[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)NB_PHILOX_M0 * c0, p1 = (uint64_t)NB_PHILOX_M1 * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += NB_PHILOX_W0;
        k1 += NB_PHILOX_W1;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// Two 32-bit draws -> two standard normals (Box-Muller): u1 in (0, 1] and u2 in [0, 1) from the top 24 bits, both exact in fp32, and
// so is the argument 2 u2 of sincospif.  The accurate library functions (no fast-math in this build).
__device__ __forceinline__ void nb_normal_pair(uint32_t a, uint32_t b, float& z_even, float& z_odd) {
    const float u1 = (float)((a >> 8) + 1u) * 0x1p-24f, u2 = (float)(b >> 8) * 0x1p-24f;
    const float r = sqrtf(-2.0f * logf(u1));
    float s, c;
    sincospif(2.0f * u2, &s, &c);
    z_even = r * c;
    z_odd = r * s;
}
