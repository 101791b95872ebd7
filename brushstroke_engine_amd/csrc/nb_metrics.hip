// Brush scores for gfx950 (metrics.BrushEvaluator): the colour and transparency metrics the reference reports per brush
// (paint_engine_metric_loop, forger/metrics/metric_main.py:153-161), on renders that are already on the device.
//
// nb_eval_masks_f32 runs once per set of drawings: `default_gaussian_smoothing` twice (forger/metrics/geom_metric.py:126-129, a 5x5
// Gaussian, sigma 1, zero padding 2 at EACH application) in one launch, and the two masks of compute_transparency_metrics
// (geom_metric.py:156-159).  A 32x32 output tile keeps the drawing with a 4-pixel halo in LDS, filters tile + 2 into a second LDS
// plane, sets what of that plane lies outside the image back to zero -- the second application pads with zeros, it does not see a
// blurred border -- and filters again.  25 taps in fp32, a convex combination of values in 0..1 per pass.
//
// nb_brush_metrics_f32 is the hot path, one launch per generator pass: what compute_lab_metrics (forger/metrics/color_metric.py:29-70)
// and the masked sums of compute_transparency_metrics state as ~25 torch launches with full-size temporaries becomes one pass over the
// render.  Per pixel: composite on white, sRGB -> linear -> XYZ -> f() -> Lab (forger/util/color.py:52-140), the distance to the
// image's target colour, and four weighted terms; NB_BRUSH_METRICS_PARTS workgroups share an image, each leaves four partial sums, and
// a second tiny launch adds an image's partials in their order.  No float atomics anywhere: the same input gives the same bits.
//
// pow(x, 2.4) is x * x * exp2(0.4 * log2 x) (the hardware log2 errs by an ulp of a value below 3.5; 0.4 of that is 7e-8 of the
// result), the cube root exp2(log2(x) / 3) with one Newton step.  Measured against float64: docs/kernel_notes.md.
//
// An image's planes are read in 16-byte vectors when every plane of the call starts on a 16-byte boundary (a render whose R * R is a
// multiple of four, in a tensor that is); otherwise pixel by pixel: the four planes of a render at R = 33 start at four different
// offsets from a boundary, and the drawing's plane at a fifth, so there is no common run of whole vectors to cut out as
// nb_select.hip does for its one row.
#include "nb_common.h"
#include <cstdint>
#include <cmath>

#define NB_EM_TILE 32
#define NB_EM_IN (NB_EM_TILE + 8)
#define NB_EM_MID (NB_EM_TILE + 4)
#define NB_BM_THREADS 256
#define NB_BM_PARTS NB_BRUSH_METRICS_PARTS

struct GaussW { float w[25]; };

__global__ __launch_bounds__(256) void eval_masks_kernel(const float* __restrict__ geom, int r, GaussW gw, float* __restrict__ blur,
                                                         uint8_t* __restrict__ mask, int32_t* n_bg, int32_t* n_fg) {
    __shared__ float in[NB_EM_IN][NB_EM_IN + 1];
    __shared__ float mid[NB_EM_MID][NB_EM_MID + 1];
    __shared__ int cnt[2];
    const int tid = threadIdx.x, k = blockIdx.z, ty0 = blockIdx.y * NB_EM_TILE, tx0 = blockIdx.x * NB_EM_TILE;
    const size_t plane = (size_t)k * (size_t)r * (size_t)r;
    for (int e = tid; e < NB_EM_IN * NB_EM_IN; e += 256) {                 // the drawing, zero outside (first application's padding)
        const int ly = e / NB_EM_IN, lx = e % NB_EM_IN, y = ty0 - 4 + ly, x = tx0 - 4 + lx;
        in[ly][lx] = (y >= 0 && y < r && x >= 0 && x < r) ? geom[plane + (size_t)y * r + x] : 0.f;
    }
    if (tid < 2) cnt[tid] = 0;
    __syncthreads();
    for (int e = tid; e < NB_EM_MID * NB_EM_MID; e += 256) {               // first application on tile + 2; zero again outside the image
        const int ly = e / NB_EM_MID, lx = e % NB_EM_MID, y = ty0 - 2 + ly, x = tx0 - 2 + lx;
        float s = 0.f;
        if (y >= 0 && y < r && x >= 0 && x < r) {
#pragma unroll
            for (int dy = 0; dy < 5; ++dy)
#pragma unroll
                for (int dx = 0; dx < 5; ++dx) s += gw.w[dy * 5 + dx] * in[ly + dy][lx + dx];
        }
        mid[ly][lx] = s;
    }
    __syncthreads();
    for (int e = tid; e < NB_EM_TILE * NB_EM_TILE; e += 256) {
        const int ly = e / NB_EM_TILE, lx = e % NB_EM_TILE, y = ty0 + ly, x = tx0 + lx;
        if (y < r && x < r) {
            float s = 0.f;
#pragma unroll
            for (int dy = 0; dy < 5; ++dy)
#pragma unroll
                for (int dx = 0; dx < 5; ++dx) s += gw.w[dy * 5 + dx] * mid[ly + dy][lx + dx];
            const bool bg = s > 0.999f, fg = in[ly + 4][lx + 4] < 0.3f;
            blur[plane + (size_t)y * r + x] = s;
            mask[plane + (size_t)y * r + x] = (uint8_t)((bg ? 1 : 0) | (fg ? 2 : 0));
            if (bg) atomicAdd(&cnt[0], 1);
            if (fg) atomicAdd(&cnt[1], 1);
        }
    }
    __syncthreads();
    if (tid == 0 && cnt[0]) atomicAdd(&n_bg[k], cnt[0]);                   // integer counts: the order of arrival does not show
    if (tid == 1 && cnt[1]) atomicAdd(&n_fg[k], cnt[1]);
}

extern "C" int nb_eval_masks_f32(const float* geom, int k, int r, float* blur, uint8_t* mask, int32_t* n_bg, int32_t* n_fg, void* stream) {
    NB_REQUIRE(geom && blur && mask && n_bg && n_fg, "eval_masks: null pointer");
    NB_REQUIRE(k >= 0 && k <= 65535 && r >= 1 && r <= 8192, "eval_masks: bad sizes (k %d outside 0..65535, r %d outside 1..8192)", k, r);
    NB_REQUIRE((((uintptr_t)geom | (uintptr_t)blur | (uintptr_t)n_bg | (uintptr_t)n_fg) & 3) == 0,
               "eval_masks: geom, blur, n_bg and n_fg must be 4-byte aligned");
    if (k == 0) return NB_OK;
    GaussW gw;
    double g[5], sum = 0.0;
    for (int i = 0; i < 5; ++i) g[i] = std::exp(-0.5 * (i - 2) * (i - 2));
    for (int i = 0; i < 25; ++i) sum += g[i / 5] * g[i % 5];
    for (int i = 0; i < 25; ++i) gw.w[i] = (float)(g[i / 5] * g[i % 5] / sum);
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(n_bg, 0, sizeof(int32_t) * (size_t)k, st) != hipSuccess || hipMemsetAsync(n_fg, 0, sizeof(int32_t) * (size_t)k, st) != hipSuccess) {
        (void)hipGetLastError();
        nb_set_error("eval_masks: clearing the counts failed");
        return NB_ELAUNCH;
    }
    const int tiles = nb_cdiv(r, NB_EM_TILE);
    hipLaunchKernelGGL(eval_masks_kernel, dim3(tiles, tiles, k), dim3(256), 0, st, geom, r, gw, blur, mask, n_bg, n_fg);
    NB_CHECK_LAUNCH("eval_masks");
    return NB_OK;
}

// ---- per-pixel colour arithmetic (forger/util/color.py:52-140) ----
__device__ __forceinline__ float bm_linear(float c) {                      // srgb2linear_rgb: the branches split at 0.04045
    const float t = (c + 0.055f) * (1.f / 1.055f);
    return c <= 0.04045f ? c * (1.f / 12.92f) : t * t * exp2f(0.4f * log2f(t));
}

__device__ __forceinline__ float bm_f(float t) {                           // xyz2lab's f(): linear below (6/29)^3, cube root of t + 1e-8 above
    const float D3 = (float)(216.0 / 24389.0), D2INV3 = (float)(841.0 / 108.0);
    const float x = t + 1.0e-8f;
    float y = exp2f(log2f(x) * (1.f / 3.f));
    const float y2 = y * y;
    y = y - (y * y2 - x) * __builtin_amdgcn_rcpf(3.f * y2);
    return t < D3 ? t * D2INV3 + (float)(4.0 / 29.0) : y;
}

__device__ __forceinline__ void bm_lab(float r, float g, float b, float& L, float& A, float& B) {
    r = bm_linear(r); g = bm_linear(g); b = bm_linear(b);
    const float X = r * 0.412453f + g * 0.357580f + b * 0.180423f;
    const float Y = r * 0.212671f + g * 0.715160f + b * 0.072169f;
    const float Z = r * 0.019334f + g * 0.119193f + b * 0.950227f;
    const float fx = bm_f(X * (float)(1.0 / 0.95047)), fy = bm_f(Y), fz = bm_f(Z * (float)(1.0 / 1.08883));
    L = 116.f * fy - 16.f;
    A = 500.f * fx - 500.f * fy;
    B = 200.f * fy - 200.f * fz;
}

struct BmParams {
    const float* renders; long long stride_n;
    const float* target; const float* geom; const uint8_t* mask;
    int k_draw, count, groups_per_part;
    float thresh; int ignore_t;
    float* alpha; float* deltas; float* partials;
};

template <int VEC> struct BmVec;
template <> struct BmVec<1> { typedef float F; typedef uint8_t M; };
template <> struct BmVec<4> { typedef float4 F; typedef uint32_t M; };

template <int VEC>
__global__ __launch_bounds__(NB_BM_THREADS) void brush_metrics_kernel(BmParams p) {
    typedef typename BmVec<VEC>::F F;
    typedef typename BmVec<VEC>::M M;
    __shared__ float tlab[3];
    __shared__ float wsum[NB_BM_THREADS / 64][4];
    const int tid = threadIdx.x, img = blockIdx.x / NB_BM_PARTS, part = blockIdx.x % NB_BM_PARTS;
    const size_t count = (size_t)p.count;
    const float* rd = p.renders + (long long)img * p.stride_n;
    const float* gd = p.geom + (size_t)(img % p.k_draw) * count;
    const uint8_t* md = p.mask + (size_t)(img % p.k_draw) * count;
    float* ad = p.alpha + (size_t)img * count;
    float* dd = p.deltas ? p.deltas + (size_t)img * count : nullptr;
    if (tid == 0) {                                                        // the target's Lab: once per workgroup, not per pixel
        float L, A, B;
        bm_lab(p.target[3 * img + 0], p.target[3 * img + 1], p.target[3 * img + 2], L, A, B);
        tlab[0] = L; tlab[1] = A; tlab[2] = B;
    }
    __syncthreads();
    const float tL = tlab[0], tA = tlab[1], tB = tlab[2];
    const int ngroups = p.count / VEC;                                     // (VEC == 4 only when count is a multiple of four)
    const int g0 = part * p.groups_per_part, g1 = min(ngroups, g0 + p.groups_per_part);
    float s_de = 0.f, s_e = 0.f, s_w = 0.f, s_bg = 0.f;
    for (int g = g0 + tid; g < g1; g += NB_BM_THREADS) {
        const size_t o = (size_t)g * VEC;
        F fr = *reinterpret_cast<const F*>(rd + o), fg = *reinterpret_cast<const F*>(rd + count + o);
        F fb = *reinterpret_cast<const F*>(rd + 2 * count + o), fa = *reinterpret_cast<const F*>(rd + 3 * count + o);
        F fgeo = *reinterpret_cast<const F*>(gd + o);
        const uint32_t m = (uint32_t)*reinterpret_cast<const M*>(md + o);
        const float* vr = reinterpret_cast<const float*>(&fr); const float* vg = reinterpret_cast<const float*>(&fg);
        const float* vb = reinterpret_cast<const float*>(&fb); const float* va = reinterpret_cast<const float*>(&fa);
        const float* vgeo = reinterpret_cast<const float*>(&fgeo);
        F fd;
        float* vd = reinterpret_cast<float*>(&fd);
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            float r = vr[j], gg = vg[j], b = vb[j];
            const float a = va[j];
            if (!p.ignore_t) {                                             // over white: alpha * rgb + (1 - alpha) * 1.0
                const float na = 1.f - a;
                r = a * r + na; gg = a * gg + na; b = a * b + na;
            }
            float L, A, B;
            bm_lab(r, gg, b, L, A, B);
            L -= tL; A -= tA; B -= tB;
            const float de = sqrtf(L * L + A * A + B * B);
            const float w = 1.f - vgeo[j];
            vd[j] = de;
            s_de += w * de;
            s_e += de > p.thresh ? w : 0.f;
            s_w += w;
            s_bg += ((m >> (8 * j)) & 1u) ? a : 0.f;
        }
        *reinterpret_cast<F*>(ad + o) = fa;
        if (dd) *reinterpret_cast<F*>(dd + o) = fd;
    }
    // fixed-order reduce: lanes by halving, then the waves one after the other
    float v[4] = {s_de, s_e, s_w, s_bg};
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) v[q] += __shfl_down(v[q], o);
    if ((tid & 63) == 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) wsum[tid >> 6][q] = v[q];
    }
    __syncthreads();
    if (tid < 4) {
        float s = wsum[0][tid];
        for (int w = 1; w < NB_BM_THREADS / 64; ++w) s += wsum[w][tid];
        p.partials[((size_t)img * NB_BM_PARTS + part) * 4 + tid] = s;
    }
}

__global__ __launch_bounds__(256) void brush_metrics_finish_kernel(const float* __restrict__ partials, int n4, float* __restrict__ sums) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= n4) return;
    const int img = t >> 2, q = t & 3;
    float s = partials[((size_t)img * NB_BM_PARTS) * 4 + q];
    for (int b = 1; b < NB_BM_PARTS; ++b) s += partials[((size_t)img * NB_BM_PARTS + b) * 4 + q];
    sums[t] = s;
}

extern "C" int nb_brush_metrics_f32(const float* renders, long long stride_n, const float* target_rgb, const float* geom,
                                    const uint8_t* mask, int k, int r, int n, float lab_thresh, int ignore_transparency,
                                    float* sums, float* alpha, float* deltas, float* partials, void* stream) {
    NB_REQUIRE(renders && target_rgb && geom && mask && sums && alpha && partials, "brush_metrics: null pointer");
    NB_REQUIRE(k >= 1 && r >= 1 && r <= 8192 && n >= 0 && n <= (1 << 24), "brush_metrics: bad sizes (k %d, r %d, n %d)", k, r, n);
    const int count = r * r;
    NB_REQUIRE(stride_n >= 4ll * count, "brush_metrics: stride_n %lld below 4 * r * r = %lld: the renders would alias", stride_n, 4ll * count);
    NB_REQUIRE((((uintptr_t)renders | (uintptr_t)target_rgb | (uintptr_t)geom | (uintptr_t)sums | (uintptr_t)alpha | (uintptr_t)deltas |
                 (uintptr_t)partials) & 3) == 0, "brush_metrics: the float pointers must be 4-byte aligned");
    if (n == 0) return NB_OK;
    const bool vec = (count & 3) == 0 && (stride_n & 3) == 0 &&
                     (((uintptr_t)renders | (uintptr_t)geom | (uintptr_t)alpha | (uintptr_t)deltas) & 15) == 0 && ((uintptr_t)mask & 3) == 0;
    const int ngroups = vec ? count / 4 : count;
    BmParams p{renders, stride_n, target_rgb, geom, mask, k, count, nb_cdiv(ngroups, NB_BM_PARTS), lab_thresh, ignore_transparency ? 1 : 0,
               alpha, deltas, partials};
    hipStream_t st = (hipStream_t)stream;
    if (vec) hipLaunchKernelGGL(brush_metrics_kernel<4>, dim3(n * NB_BM_PARTS), dim3(NB_BM_THREADS), 0, st, p);
    else hipLaunchKernelGGL(brush_metrics_kernel<1>, dim3(n * NB_BM_PARTS), dim3(NB_BM_THREADS), 0, st, p);
    NB_CHECK_LAUNCH("brush_metrics");
    hipLaunchKernelGGL(brush_metrics_finish_kernel, dim3(nb_cdiv(4 * n, 256)), dim3(256), 0, st, (const float*)partials, 4 * n, sums);
    NB_CHECK_LAUNCH("brush_metrics_finish");
    return NB_OK;
}
