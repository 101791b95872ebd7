// A projected brush's noise as a device object (include/neube_hip.h, "brush noise sets"): every synthesis layer's noise_const
// replacement and its transpose, written to fixed addresses by ONE launch.  The reference's brush libraries store the buffers the
// projection optimised beside ws (forger/ui/library.py:146-202) and, between two brushes, their lerp
// (formats.WBrushLibrary.set_interpolated_style); the generator reads them where it reads noise_const (networks.py:372-382), and
// the convolutions that compute their shifted noise themselves read the transpose (NbNoiseSrc).
#include "nb_common.h"

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
