// Seeded random noise of every synthesis layer in one launch (SynthesisLayer's noise_mode 'random', training/networks.py:369-370,
// with a counter-based generator in place of torch.randn): the draw is a pure function of (seed, sample, layer, pixel), so a sample
// gets the same noise at any batch size, on any rank, from Python or C, and in a graph replay.  include/neube_hip.h states the
// generator; tests/philox_ref.py restates it in numpy.
#include "nb_common.h"
#include <algorithm>

#include "nb_philox.h"      // Philox4x32-10 and the Box-Muller pair (shared with csrc/nb_drawings.hip)

// One thread = one Philox call = one pixel quad (four normals, one 16-byte store); lanes run along q.  blockIdx.y = table row,
// blockIdx.z = sample; a block walks quads blockIdx.x * 256 + t, + gridDim.x * 256, ... of its (layer, sample), so the values do
// not depend on the grid: blocks beyond a small layer's quads leave at once, a capped grid strides over a large one.
__global__ __launch_bounds__(256) void noise_seeded_kernel(const NbLayerDesc* __restrict__ layers, int first_layer, uint64_t seed,
                                                           uint64_t offset, const uint64_t* __restrict__ state) {
    const NbLayerDesc L = layers[blockIdx.y];
    if (!L.noise_out) return;
    if (state) {
        seed = state[0];
        offset = state[1];
    }
    const uint32_t npix = (uint32_t)L.res * (uint32_t)L.res, quads = (npix + 3u) / 4u;
    const uint64_t s = offset + blockIdx.z;
    const uint32_t layer = (uint32_t)(first_layer + (int)blockIdx.y);
    float* __restrict__ out = L.noise_out + (size_t)blockIdx.z * npix;
    const bool scaled = L.noise_strength != nullptr;
    const float strength = scaled ? L.noise_strength[0] : 1.f;
    for (uint32_t q = blockIdx.x * 256u + threadIdx.x; q < quads; q += gridDim.x * 256u) {
        uint32_t x[4];
        nb_philox4x32_10(q, layer, (uint32_t)s, (uint32_t)(s >> 32), (uint32_t)seed, (uint32_t)(seed >> 32), x);
        float z[4];
        nb_normal_pair(x[0], x[1], z[0], z[1]);
        nb_normal_pair(x[2], x[3], z[2], z[3]);
        if (scaled) {
#pragma unroll
            for (int e = 0; e < 4; ++e) z[e] = z[e] * strength;
        }
        float* p = out + (size_t)q * 4;
        if (q * 4u + 3u < npix && (reinterpret_cast<uintptr_t>(p) & 15u) == 0) {
            *reinterpret_cast<float4*>(p) = make_float4(z[0], z[1], z[2], z[3]);
        } else {
            // the ragged last quad of an image whose size is no multiple of 4, and every quad of such an image's later samples
            // (their base is not 16-byte aligned): only the pixels that exist
#pragma unroll
            for (uint32_t e = 0; e < 4; ++e)
                if (q * 4u + e < npix) p[e] = z[e];
        }
    }
}

extern "C" int nb_noise_seeded_f32(const NbLayerDesc* layers_dev, int first_layer, int n_layers, int max_res, uint64_t seed,
                                   uint64_t offset, const uint64_t* state_dev, int n, void* stream) {
    NB_REQUIRE(layers_dev, "noise_seeded: null pointer");
    NB_REQUIRE(first_layer >= 0 && n_layers >= 1 && n_layers <= 65535 && max_res >= 1 && max_res <= 32768 && n >= 1 && n <= 65535,
               "noise_seeded: bad sizes");
    // blocks per (layer, sample): enough for the largest layer, capped so that the whole grid stays near 8192 blocks (a small layer
    // is one partly filled wave, and tens of thousands of empty blocks cost more than the work); the kernel strides over the rest
    const long long quads = ((long long)max_res * max_res + 3) / 4;
    const long long want = (quads + 255) / 256, cap = std::max(1LL, 8192LL / ((long long)n_layers * n));
    dim3 grid((unsigned)std::min(want, cap), n_layers, n);
    hipLaunchKernelGGL(noise_seeded_kernel, grid, dim3(256), 0, (hipStream_t)stream, layers_dev, first_layer, seed, offset, state_dev);
    NB_CHECK_LAUNCH("noise_seeded");
    return NB_OK;
}
