// A projected brush's noise as a device object (include/neube_hip.h, "brush noise sets"): every synthesis layer's noise_const
// replacement and its transpose, written to fixed addresses by ONE launch.  The reference's brush libraries store the buffers the
// projection optimised beside ws (forger/ui/library.py:146-202) and, between two brushes, their lerp
// (formats.WBrushLibrary.set_interpolated_style); the generator reads them where it reads noise_const (networks.py:372-382), and
// the convolutions that compute their shifted noise themselves read the transpose (NbNoiseSrc).  Below the kernel: the sets a
// generator handle owns and binds (nb_brush_noise_create / _load / _destroy, nb_generator_bind_brush_noise).
#include "nb_gen_internal.h"

namespace {

// the kernel's argument block (by value, ~1.1 KB of the kernarg segment): the layers, and the running tile count behind each
struct BrushNoiseArgs {
    NbBrushNoiseLayer L[NB_PLAN_MAX_LAYERS];
    int tile_end[NB_PLAN_MAX_LAYERS];
    int n_layers;
    float wa, wb;
};

constexpr int kTile = 32;

}  // namespace

// One workgroup = one 32 x 32 tile of one layer (256 threads: 32 columns x 8 rows, four rows per thread).  Rows of `a` / `b` are read
// and rows of `dst` written with the lanes along x; the tile then goes through LDS and rows of `dst_t` are written with the lanes
// along the source's y.  The LDS row is padded to 33 floats: a 32-lane half writes one row (banks x) and reads one column (banks
// (33 x + r) mod 32 = x + r): both conflict free under the 32-bank rule of ds_write_b32 / ds_read_b32.  Layers smaller than a tile
// (4, 8, 16) are one partly filled tile: every access is bounded by res.  `dst` may be `a` (each thread reads and writes its own
// elements); `dst_t` aliases neither input (checked by the caller of the entry, stated in the header).
__global__ __launch_bounds__(256) void brush_noise_build_kernel(const BrushNoiseArgs A) {
    __shared__ float tile[kTile][kTile + 1];
    int l = 0;
    while (l + 1 < A.n_layers && (int)blockIdx.x >= A.tile_end[l]) ++l;
    const NbBrushNoiseLayer L = A.L[l];
    const int t = (int)blockIdx.x - (l ? A.tile_end[l - 1] : 0);
    const int res = L.res, per_row = (res + kTile - 1) / kTile;
    const int y0 = (t / per_row) * kTile, x0 = (t % per_row) * kTile;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const float* a = L.a;
    const float* b = L.b;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int r = ty + 8 * k, y = y0 + r, x = x0 + tx;
        if (y < res && x < res) {
            const size_t idx = (size_t)y * res + x;
            float v = a[idx];
            // two rounded products, one rounded sum, no FMA: the host's float32 `a * alpha + b * (1 - alpha)`
            if (b) v = __fadd_rn(__fmul_rn(v, A.wa), __fmul_rn(b[idx], A.wb));
            L.dst[idx] = v;
            tile[r][tx] = v;
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int r = ty + 8 * k, x = x0 + r, y = y0 + tx;      // dst_t[x, y] = dst[y, x] = tile[y - y0][x - x0]
        if (x < res && y < res) L.dst_t[(size_t)x * res + y] = tile[tx][r];
    }
}

extern "C" int nb_brush_noise_build_f32(const NbBrushNoiseLayer* layers_host, int n_layers, float wa, float wb, void* stream) {
    NB_REQUIRE(layers_host, "brush_noise_build: null layer array");
    NB_REQUIRE(n_layers >= 1 && n_layers <= NB_PLAN_MAX_LAYERS, "brush_noise_build: %d layers outside [1, %d]", n_layers, NB_PLAN_MAX_LAYERS);
    BrushNoiseArgs args{};
    int tiles = 0;
    for (int i = 0; i < n_layers; ++i) {
        const NbBrushNoiseLayer& L = layers_host[i];
        NB_REQUIRE(L.a && L.dst && L.dst_t, "brush_noise_build: layer %d has a null a / dst / dst_t", i);
        NB_REQUIRE(L.res >= 4 && L.res <= 32768 && (L.res & (L.res - 1)) == 0,
                   "brush_noise_build: layer %d: res %d is not a power of two in [4, 32768]", i, L.res);
        NB_REQUIRE((const float*)L.dst_t != L.a && (const float*)L.dst_t != L.b && L.dst_t != L.dst,
                   "brush_noise_build: layer %d: dst_t aliases a, b or dst", i);
        const int per_row = (L.res + kTile - 1) / kTile;
        tiles += per_row * per_row;
        args.L[i] = L;
        args.tile_end[i] = tiles;
    }
    args.n_layers = n_layers;
    args.wa = wa;
    args.wb = wb;
    hipLaunchKernelGGL(brush_noise_build_kernel, dim3(tiles), dim3(256), 0, (hipStream_t)stream, args);
    NB_CHECK_LAUNCH("brush_noise_build");
    return NB_OK;
}

// ------------------------------------------------------------------------------------------------
// brush noise sets: a projected brush's noise_const replacements and their transposes at fixed addresses (include/neube_hip.h)
// ------------------------------------------------------------------------------------------------
using namespace nbgen;

namespace {

void brush_noise_free(NbBrushNoise* bn, int device) {
    if (bn->buf || bn->tables) {
        const DeviceScope scope(device);
        if (scope.ok) {
            (void)hipDeviceSynchronize();
            if (bn->buf) (void)hipFree(bn->buf);
            if (bn->tables) (void)hipFree(bn->tables);
        }
    }
    delete bn;
}

// one nb_brush_noise_build_f32 launch into the set; a NULL a[i] / b[i] is the checkpoint's buffer, b == NULL a plain copy
int brush_noise_fill(NbBrushNoise* bn, const float* const* a, const float* const* b, float wa, float wb, void* stream) {
    const NbGenerator* g = bn->gen;
    const int nL = (int)g->L.size();
    NbBrushNoiseLayer layers[NB_PLAN_MAX_LAYERS];
    for (int i = 0; i < nL; ++i) {
        const float* ck = g->L[i].noise_const;
        layers[i] = NbBrushNoiseLayer{a && a[i] ? a[i] : ck, b ? (b[i] ? b[i] : ck) : nullptr, bn->nc[i], bn->nc_t[i],
                                      g->cfg.layers[i].block_res, 0};
    }
    return nb_brush_noise_build_f32(layers, nL, wa, wb, stream);
}

}  // namespace

extern "C" int nb_brush_noise_create(NbGenerator* gen, void* stream, NbBrushNoise** out) {
    NB_REQUIRE(out, "brush_noise_create: null output handle");
    *out = nullptr;
    NB_REQUIRE(gen, "brush_noise_create: null generator");
    if (const int rc = require_current_device(gen, "brush_noise_create")) return rc;
    const int nL = (int)gen->L.size();
    size_t floats = 0;
    // (every image on a 256-byte boundary, as the checkpoint's own copies are)
    auto padded = [](const GenLayer& s) { return ((size_t)s.block_res * s.block_res + 63) / 64 * 64; };
    for (const GenLayer& s : gen->cfg.layers) floats += 2 * padded(s);
    NbBrushNoise* bn = new NbBrushNoise();
    bn->gen = gen;
    const size_t table_bytes = gen->host_tables.size() * sizeof(NbLayerDesc);
    if (hipMalloc((void**)&bn->buf, floats * sizeof(float)) != hipSuccess || hipMalloc((void**)&bn->tables, table_bytes) != hipSuccess) {
        nb_set_error("brush_noise_create: hipMalloc of %zu bytes failed", floats * sizeof(float) + table_bytes);
        brush_noise_free(bn, gen->device);
        return NB_ELAUNCH;
    }
    float* p = bn->buf;
    for (const GenLayer& s : gen->cfg.layers) {
        bn->nc.push_back(p);
        bn->nc_t.push_back(p + padded(s));
        p += 2 * padded(s);
    }
    // the handle's tables with noise_const pointing into the set (where a table has it cleared it stays cleared)
    std::vector<NbLayerDesc> descs = gen->host_tables;
    for (int first = 0; first <= nL; ++first)
        for (int i = 0; i < nL; ++i) {
            NbLayerDesc& d = descs[(size_t)first * (nL + 1) + i];
            if (d.noise_const) d.noise_const = bn->nc[i];
        }
    int rc = brush_noise_fill(bn, nullptr, nullptr, 1.f, 0.f, stream);
    if (rc == NB_OK && (hipMemcpyAsync(bn->tables, descs.data(), table_bytes, hipMemcpyHostToDevice, (hipStream_t)stream) != hipSuccess ||
                        hipStreamSynchronize((hipStream_t)stream) != hipSuccess)) {
        nb_set_error("brush_noise_create: %s", hipGetErrorString(hipGetLastError()));
        rc = NB_ELAUNCH;
    }
    if (rc != NB_OK) {
        brush_noise_free(bn, gen->device);
        return rc;
    }
    gen->sets.push_back(bn);
    *out = bn;
    return NB_OK;
}

extern "C" int nb_brush_noise_load(NbBrushNoise* bn, const float* const* a_dev, const float* const* b_dev, float alpha, void* stream) {
    NB_REQUIRE(bn, "brush_noise_load: null set");
    NB_REQUIRE(bn->gen, "brush_noise_load: the set's generator has been destroyed");
    NB_REQUIRE(a_dev, "brush_noise_load: null buffer array (a NULL entry stands for the checkpoint's buffer, the array itself may not be NULL)");
    if (const int rc = require_current_device(bn->gen, "brush_noise_load")) return rc;
    return brush_noise_fill(bn, a_dev, b_dev, alpha, (float)(1.0 - (double)alpha), stream);
}

extern "C" int nb_generator_bind_brush_noise(NbGenerator* gen, NbBrushNoise* bn) {
    NB_REQUIRE(gen, "generator_bind_brush_noise: null generator");
    NB_REQUIRE(!bn || bn->gen == gen, "generator_bind_brush_noise: the set belongs to another generator");
    gen->brush = bn;
    return NB_OK;
}

extern "C" int nb_brush_noise_destroy(NbBrushNoise* bn) {
    if (!bn) return NB_OK;
    int device = 0;
    if (NbGenerator* g = bn->gen) {
        device = g->device;
        if (g->brush == bn) g->brush = nullptr;
        for (size_t k = 0; k < g->sets.size(); ++k)
            if (g->sets[k] == bn) {
                g->sets.erase(g->sets.begin() + k);
                break;
            }
    } else {
        (void)hipGetDevice(&device);              // (an orphan: its generator went first, on the device that was current then)
    }
    brush_noise_free(bn, device);
    return NB_OK;
}
