// Inputs of the perceptual brush scores for gfx950 (metrics.BrushEvaluator with an LPIPS network): what
// compute_uniform_bg_lpips_metric (forger/metrics/geom_metric.py:207-262) and compute_lpips_across_geo (geom_metric.py:190-204) do
// to a batch of renders BEFORE the network sees it -- composite over white, one Gaussian blur of the guidance, the masked mean
// colour, two crops (the second transposed and perhaps permuted), the joint background mask, the fill with the mean colour, the
// rescale to -1..1: about thirty torch launches with full-size temporaries per call there, three kernels here.
//
// nb_bg_guidance_f32 runs once per set of drawings: `default_gaussian_smoothing` ONCE (geom_metric.py:235; 5x5, sigma 1, zero
// padding 2, the weights of nb_eval_masks_f32) and the number of pixels above BG_THRESH = 0.99 (geom_metric.py:238-239).  A 32x32
// output tile keeps the drawing with a 2-pixel halo in LDS.
//
// nb_bg_mean_colors_f32 is one pass over the renders: the on-white colour summed where the blurred guidance exceeds 0.99
// (geom_metric.py:232-241).  NB_BG_MEAN_PARTS workgroups share an image and leave three partial sums each; a small second launch
// adds an image's partials in their order and divides by max(n_bg, 1).  16-byte vectors when every plane of the call is aligned,
// pixel by pixel otherwise, as nb_brush_metrics_f32.
//
// nb_metric_pairs_f32 is the hot path, one launch per metric and pass: it writes the network's input of both sides of every pair
// into one buffer.  A workgroup owns a 32x32 tile of ONE pair's output -- both patches, because the mask joins them.  The first patch
// is read where it lies, 32 consecutive lanes along a row.  The second patch is transposed (geom_metric.py:250): output pixel (y, x)
// comes from source pixel (x, y) of the window, so the tile's SOURCE is the 32x32 block at (x0, y0) of the window.  Read by output
// pixel that would be 32 lanes walking down a column, r floats apart, one 64-byte request each.  So the source block is read along its
// rows, composited over white on the way, and staged as four planes (r, g, b on white, blurred guidance) of 32 x 33 floats in LDS;
// the transposed read then goes down an LDS column.  With the row pitch 33, ds_write_b32 / ds_read_b32 (32 banks of 4 bytes, conflicts
// counted within a 32-lane half) see 32 different banks either way: lanes along a row differ by 1, lanes down a column by 33 = 1 mod 32.
//
// Windows start at any column and p is usually odd (int(0.8 r): 51 at r = 64, 26 at r = 33), so neither the window rows nor the
// output planes have 16-byte runs in common across a launch; the general path moves 4-byte elements, a 128-byte row segment per 32
// lanes.  When p, r and the sample stride are multiples of four and renders, blur1 and out are 16-byte aligned (p = 64 at r = 128 or
// 256; the across-drawing form, which is not transposed, at such r), every thread owns four consecutive output columns and stores 16-byte vectors, and reads
// 16-byte vectors from a window whose column offset is a multiple of four (decided per pair, uniform over the workgroup).
//
// Offsets and src1 live on the device and cannot be validated on the host: the kernel clamps an offset into 0..r - p and an index
// into 0..n - 1, so a bad plan gives a wrong patch, never a read outside the renders.  No float atomics anywhere.
#include "nb_common.h"
#include <cstdint>
#include <cmath>

#define NB_MP_TILE 32
#define NB_MP_PITCH (NB_MP_TILE + 1)
#define NB_MP_THREADS 256
#define NB_BGM_THREADS 256
#define NB_BGM_PARTS NB_BG_MEAN_PARTS
#define NB_BGG_IN (NB_MP_TILE + 4)
#define NB_BG_THRESH 0.99f

struct MpGaussW { float w[25]; };

__global__ __launch_bounds__(256) void bg_guidance_kernel(const float* __restrict__ geom, int r, MpGaussW gw, float* __restrict__ blur1,
                                                          int32_t* n_bg) {
    __shared__ float in[NB_BGG_IN][NB_BGG_IN + 1];
    __shared__ int cnt;
    const int tid = threadIdx.x, k = blockIdx.z, ty0 = blockIdx.y * NB_MP_TILE, tx0 = blockIdx.x * NB_MP_TILE;
    const size_t plane = (size_t)k * (size_t)r * (size_t)r;
    for (int e = tid; e < NB_BGG_IN * NB_BGG_IN; e += 256) {               // the drawing, zero outside (the padding)
        const int ly = e / NB_BGG_IN, lx = e % NB_BGG_IN, y = ty0 - 2 + ly, x = tx0 - 2 + lx;
        in[ly][lx] = (y >= 0 && y < r && x >= 0 && x < r) ? geom[plane + (size_t)y * r + x] : 0.f;
    }
    if (tid == 0) cnt = 0;
    __syncthreads();
    for (int e = tid; e < NB_MP_TILE * NB_MP_TILE; e += 256) {
        const int ly = e / NB_MP_TILE, lx = e % NB_MP_TILE, y = ty0 + ly, x = tx0 + lx;
        if (y < r && x < r) {
            float s = 0.f;
#pragma unroll
            for (int dy = 0; dy < 5; ++dy)
#pragma unroll
                for (int dx = 0; dx < 5; ++dx) s += gw.w[dy * 5 + dx] * in[ly + dy][lx + dx];
            blur1[plane + (size_t)y * r + x] = s;
            if (s > NB_BG_THRESH) atomicAdd(&cnt, 1);
        }
    }
    __syncthreads();
    if (tid == 0 && cnt) atomicAdd(&n_bg[k], cnt);                         // integer counts: the order of arrival does not show
}

extern "C" int nb_bg_guidance_f32(const float* geom, int k, int r, float* blur1, int32_t* n_bg, void* stream) {
    NB_REQUIRE(geom && blur1 && n_bg, "bg_guidance: null pointer");
    NB_REQUIRE(k >= 0 && k <= 65535 && r >= 1 && r <= 8192, "bg_guidance: bad sizes (k %d outside 0..65535, r %d outside 1..8192)", k, r);
    NB_REQUIRE((((uintptr_t)geom | (uintptr_t)blur1 | (uintptr_t)n_bg) & 3) == 0, "bg_guidance: geom, blur1 and n_bg must be 4-byte aligned");
    if (k == 0) return NB_OK;
    MpGaussW gw;
    double g[5], sum = 0.0;
    for (int i = 0; i < 5; ++i) g[i] = std::exp(-0.5 * (i - 2) * (i - 2));
    for (int i = 0; i < 25; ++i) sum += g[i / 5] * g[i % 5];
    for (int i = 0; i < 25; ++i) gw.w[i] = (float)(g[i / 5] * g[i % 5] / sum);
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(n_bg, 0, sizeof(int32_t) * (size_t)k, st) != hipSuccess) {
        (void)hipGetLastError();
        nb_set_error("bg_guidance: clearing the counts failed");
        return NB_ELAUNCH;
    }
    const int tiles = nb_cdiv(r, NB_MP_TILE);
    hipLaunchKernelGGL(bg_guidance_kernel, dim3(tiles, tiles, k), dim3(256), 0, st, geom, r, gw, blur1, n_bg);
    NB_CHECK_LAUNCH("bg_guidance");
    return NB_OK;
}

// ---- masked mean colour ----
struct BgmParams {
    const float* renders; long long stride_n;
    const float* blur1;
    int k_draw, count, groups_per_part;
    float* partials;
};

template <int VEC> struct MpVec;
template <> struct MpVec<1> { typedef float F; };
template <> struct MpVec<4> { typedef float4 F; };

template <int VEC>
__global__ __launch_bounds__(NB_BGM_THREADS) void bg_mean_kernel(BgmParams p) {
    typedef typename MpVec<VEC>::F F;
    __shared__ float wsum[NB_BGM_THREADS / 64][3];
    const int tid = threadIdx.x, img = blockIdx.x / NB_BGM_PARTS, part = blockIdx.x % NB_BGM_PARTS;
    const size_t count = (size_t)p.count;
    const float* rd = p.renders + (long long)img * p.stride_n;
    const float* bd = p.blur1 + (size_t)(img % p.k_draw) * count;
    const int ngroups = p.count / VEC;                                     // (VEC == 4 only when count is a multiple of four)
    const int g0 = part * p.groups_per_part, g1 = min(ngroups, g0 + p.groups_per_part);
    float v[3] = {0.f, 0.f, 0.f};
    for (int g = g0 + tid; g < g1; g += NB_BGM_THREADS) {
        const size_t o = (size_t)g * VEC;
        F fr = *reinterpret_cast<const F*>(rd + o), fg = *reinterpret_cast<const F*>(rd + count + o);
        F fb = *reinterpret_cast<const F*>(rd + 2 * count + o), fa = *reinterpret_cast<const F*>(rd + 3 * count + o);
        F fm = *reinterpret_cast<const F*>(bd + o);
        const float* vr = reinterpret_cast<const float*>(&fr); const float* vg = reinterpret_cast<const float*>(&fg);
        const float* vb = reinterpret_cast<const float*>(&fb); const float* va = reinterpret_cast<const float*>(&fa);
        const float* vm = reinterpret_cast<const float*>(&fm);
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            const float a = va[j], na = 1.f - a;                           // over white: alpha * rgb + (1 - alpha) * 1.0
            const bool bg = vm[j] > NB_BG_THRESH;
            v[0] += bg ? a * vr[j] + na : 0.f;
            v[1] += bg ? a * vg[j] + na : 0.f;
            v[2] += bg ? a * vb[j] + na : 0.f;
        }
    }
    // fixed-order reduce: lanes by halving, then the waves one after the other
#pragma unroll
    for (int q = 0; q < 3; ++q)
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) v[q] += __shfl_down(v[q], o);
    if ((tid & 63) == 0) {
#pragma unroll
        for (int q = 0; q < 3; ++q) wsum[tid >> 6][q] = v[q];
    }
    __syncthreads();
    if (tid < 3) {
        float s = wsum[0][tid];
        for (int w = 1; w < NB_BGM_THREADS / 64; ++w) s += wsum[w][tid];
        p.partials[((size_t)img * NB_BGM_PARTS + part) * 3 + tid] = s;
    }
}

__global__ __launch_bounds__(256) void bg_mean_finish_kernel(const float* __restrict__ partials, const int32_t* __restrict__ n_bg, int k_draw,
                                                             int n3, float* __restrict__ mean) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= n3) return;
    const int img = t / 3, q = t % 3;
    float s = partials[((size_t)img * NB_BGM_PARTS) * 3 + q];
    for (int b = 1; b < NB_BGM_PARTS; ++b) s += partials[((size_t)img * NB_BGM_PARTS + b) * 3 + q];
    mean[t] = s / (float)max(n_bg[img % k_draw], 1);
}

extern "C" int nb_bg_mean_colors_f32(const float* renders, long long stride_n, const float* blur1, const int32_t* n_bg, int k, int r, int n,
                                     float* partials, float* mean, void* stream) {
    NB_REQUIRE(renders && blur1 && n_bg && partials && mean, "bg_mean_colors: null pointer");
    NB_REQUIRE(k >= 1 && r >= 1 && r <= 8192 && n >= 0 && n <= (1 << 24), "bg_mean_colors: bad sizes (k %d, r %d, n %d)", k, r, n);
    const int count = r * r;
    NB_REQUIRE(stride_n >= 4ll * count, "bg_mean_colors: stride_n %lld below 4 * r * r = %lld: the renders would alias", stride_n, 4ll * count);
    NB_REQUIRE((((uintptr_t)renders | (uintptr_t)blur1 | (uintptr_t)n_bg | (uintptr_t)partials | (uintptr_t)mean) & 3) == 0,
               "bg_mean_colors: the float and int pointers must be 4-byte aligned");
    if (n == 0) return NB_OK;
    const bool vec = (count & 3) == 0 && (stride_n & 3) == 0 && (((uintptr_t)renders | (uintptr_t)blur1) & 15) == 0;
    const int ngroups = vec ? count / 4 : count;
    BgmParams p{renders, stride_n, blur1, k, count, nb_cdiv(ngroups, NB_BGM_PARTS), partials};
    hipStream_t st = (hipStream_t)stream;
    if (vec) hipLaunchKernelGGL(bg_mean_kernel<4>, dim3(n * NB_BGM_PARTS), dim3(NB_BGM_THREADS), 0, st, p);
    else hipLaunchKernelGGL(bg_mean_kernel<1>, dim3(n * NB_BGM_PARTS), dim3(NB_BGM_THREADS), 0, st, p);
    NB_CHECK_LAUNCH("bg_mean_colors");
    hipLaunchKernelGGL(bg_mean_finish_kernel, dim3(nb_cdiv(3 * n, 256)), dim3(256), 0, st, (const float*)partials, n_bg, k, 3 * n, mean);
    NB_CHECK_LAUNCH("bg_mean_colors_finish");
    return NB_OK;
}

// ---- the pairs ----
struct MpParams {
    const float* renders; long long stride_n;
    const float* blur1; const float* mean;
    const int32_t* off0; const int32_t* off1; const int32_t* src1;
    int k_draw, r, p, n, tiles, masked;
    float* out;
};

// G floats from q: one 16-byte vector where the run is aligned, else element by element
template <int G>
__device__ __forceinline__ void mp_load(const float* q, bool aligned, float (&v)[G]) {
    if (G == 4 && aligned) {
        const float4 f = *reinterpret_cast<const float4*>(q);
        v[0] = f.x; v[1 % G] = f.y; v[2 % G] = f.z; v[3 % G] = f.w;
    } else {
#pragma unroll
        for (int j = 0; j < G; ++j) v[j] = q[j];
    }
}

template <int G>
__device__ __forceinline__ void mp_store(float* q, const float (&v)[G]) {
    if (G == 4) *reinterpret_cast<float4*>(q) = make_float4(v[0], v[1 % G], v[2 % G], v[3 % G]);
    else q[0] = v[0];
}

// G: output columns per thread (4: the 16-byte path).  TR: the second patch is transposed.
template <int G, bool TR>
__global__ __launch_bounds__(NB_MP_THREADS) void metric_pairs_kernel(MpParams P) {
    __shared__ float st[TR ? 4 : 1][TR ? NB_MP_TILE : 1][TR ? NB_MP_PITCH : 1];
    const int tid = threadIdx.x, r = P.r, p = P.p;
    const int i = blockIdx.x / (P.tiles * P.tiles), t = blockIdx.x % (P.tiles * P.tiles);
    const int y0 = (t / P.tiles) * NB_MP_TILE, x0 = (t % P.tiles) * NB_MP_TILE;
    const size_t count = (size_t)r * r, pcount = (size_t)p * p;
    const int lim = r - p;
    const int j = P.src1 ? min(max(P.src1[i], 0), P.n - 1) : i;
    const int o0r = min(max(P.off0[2 * i], 0), lim), o0c = min(max(P.off0[2 * i + 1], 0), lim);
    const int o1r = min(max(P.off1[2 * i], 0), lim), o1c = min(max(P.off1[2 * i + 1], 0), lim);
    const float* r0 = P.renders + (long long)i * P.stride_n;
    const float* r1 = P.renders + (long long)j * P.stride_n;
    const float* b0 = P.blur1 + (size_t)(i % P.k_draw) * count;
    const float* b1 = P.blur1 + (size_t)(j % P.k_draw) * count;
    // the FIRST image's mean for both patches (geom_metric.py:256-257)
    const float m0 = P.masked ? P.mean[3 * i] : 0.f, m1 = P.masked ? P.mean[3 * i + 1] : 0.f, m2 = P.masked ? P.mean[3 * i + 2] : 0.f;
    const bool al0 = (o0c & 3) == 0, al1 = (o1c & 3) == 0;                 // (x0, lx are multiples of four on the G == 4 path)
    constexpr int COLS = NB_MP_TILE / G, PASSES = NB_MP_TILE * COLS / NB_MP_THREADS;

    if (TR) {
        // the source block of the second patch: window rows x0 .. x0 + 31, window columns y0 .. y0 + 31, read along its rows
#pragma unroll
        for (int it = 0; it < PASSES; ++it) {
            const int e = tid + it * NB_MP_THREADS, sy = e / COLS, sx = (e % COLS) * G;         // sy: window row - x0, sx: window column - y0
            if (x0 + sy < p && y0 + sx < p) {                              // (G == 4: p is a multiple of four, a group is inside or outside)
                const size_t o = (size_t)(o1r + x0 + sy) * r + (size_t)(o1c + y0 + sx);
                float cr[G], cg[G], cb[G], ca[G], cm[G];
                mp_load<G>(r1 + o, al1, cr); mp_load<G>(r1 + count + o, al1, cg); mp_load<G>(r1 + 2 * count + o, al1, cb);
                mp_load<G>(r1 + 3 * count + o, al1, ca);
#pragma unroll
                for (int q = 0; q < G; ++q) cm[q] = 0.f;
                if (P.masked) mp_load<G>(b1 + o, al1, cm);
#pragma unroll
                for (int q = 0; q < G; ++q) {
                    const float a = ca[q], na = 1.f - a;
                    st[0][sy][sx + q] = a * cr[q] + na;
                    st[1][sy][sx + q] = a * cg[q] + na;
                    st[2][sy][sx + q] = a * cb[q] + na;
                    st[3][sy][sx + q] = cm[q];
                }
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int it = 0; it < PASSES; ++it) {
        const int e = tid + it * NB_MP_THREADS, ly = e / COLS, lx = (e % COLS) * G, y = y0 + ly, x = x0 + lx;
        if (y >= p || x >= p) continue;
        const size_t o = (size_t)(o0r + y) * r + (size_t)(o0c + x);
        float cr[G], cg[G], cb[G], ca[G], cm[G], s[3][G], sm[G];
        mp_load<G>(r0 + o, al0, cr); mp_load<G>(r0 + count + o, al0, cg); mp_load<G>(r0 + 2 * count + o, al0, cb);
        mp_load<G>(r0 + 3 * count + o, al0, ca);
#pragma unroll
        for (int q = 0; q < G; ++q) cm[q] = sm[q] = 0.f;
        if (P.masked) mp_load<G>(b0 + o, al0, cm);
        if (TR) {
#pragma unroll
            for (int q = 0; q < G; ++q) {
                s[0][q] = st[0][lx + q][ly]; s[1][q] = st[1][lx + q][ly]; s[2][q] = st[2][lx + q][ly]; sm[q] = st[3][lx + q][ly];
            }
        } else {
            const size_t o1 = (size_t)(o1r + y) * r + (size_t)(o1c + x);
            float dr[G], dg[G], db[G], da[G];
            mp_load<G>(r1 + o1, al1, dr); mp_load<G>(r1 + count + o1, al1, dg); mp_load<G>(r1 + 2 * count + o1, al1, db);
            mp_load<G>(r1 + 3 * count + o1, al1, da);
            if (P.masked) mp_load<G>(b1 + o1, al1, sm);
#pragma unroll
            for (int q = 0; q < G; ++q) {
                const float a = da[q], na = 1.f - a;
                s[0][q] = a * dr[q] + na; s[1][q] = a * dg[q] + na; s[2][q] = a * db[q] + na;
            }
        }
        float f[3][G], g[3][G];
#pragma unroll
        for (int q = 0; q < G; ++q) {
            const float a = ca[q], na = 1.f - a;
            const bool keep = !P.masked || (cm[q] > NB_BG_THRESH && sm[q] > NB_BG_THRESH);       // background in BOTH patches
            f[0][q] = (keep ? a * cr[q] + na : m0) * 2.f - 1.f;
            f[1][q] = (keep ? a * cg[q] + na : m1) * 2.f - 1.f;
            f[2][q] = (keep ? a * cb[q] + na : m2) * 2.f - 1.f;
            g[0][q] = (keep ? s[0][q] : m0) * 2.f - 1.f;
            g[1][q] = (keep ? s[1][q] : m1) * 2.f - 1.f;
            g[2][q] = (keep ? s[2][q] : m2) * 2.f - 1.f;
        }
        const size_t po = (size_t)y * p + x;
        float* d0 = P.out + (size_t)i * 3 * pcount + po;
        float* d1 = P.out + ((size_t)P.n + i) * 3 * pcount + po;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            mp_store<G>(d0 + c * pcount, f[c]);
            mp_store<G>(d1 + c * pcount, g[c]);
        }
    }
}

extern "C" int nb_metric_pairs_f32(const float* renders, long long stride_n, const float* blur1, const float* mean, const int32_t* off0,
                                   const int32_t* off1, const int32_t* src1, int k, int r, int p, int n, int flags, float* out, void* stream) {
    const bool masked = (flags & NB_METRIC_PAIRS_MASKED) != 0, tr = (flags & NB_METRIC_PAIRS_TRANSPOSE) != 0;
    NB_REQUIRE(renders && off0 && off1 && out, "metric_pairs: null pointer");
    NB_REQUIRE(!masked || (blur1 && mean), "metric_pairs: MASKED needs blur1 and mean");
    NB_REQUIRE((flags & ~(NB_METRIC_PAIRS_MASKED | NB_METRIC_PAIRS_TRANSPOSE)) == 0, "metric_pairs: unknown flags 0x%x", flags);
    NB_REQUIRE(k >= 1 && r >= 1 && r <= 8192 && p >= 1 && p <= r && n >= 0 && n <= (1 << 24), "metric_pairs: bad sizes (k %d, r %d, p %d, n %d)",
               k, r, p, n);
    const long long count = (long long)r * r;
    NB_REQUIRE(stride_n >= 4 * count, "metric_pairs: stride_n %lld below 4 * r * r = %lld: the renders would alias", stride_n, 4 * count);
    NB_REQUIRE((((uintptr_t)renders | (uintptr_t)blur1 | (uintptr_t)mean | (uintptr_t)off0 | (uintptr_t)off1 | (uintptr_t)src1 | (uintptr_t)out) & 3) == 0,
               "metric_pairs: the float and int pointers must be 4-byte aligned");
    const int tiles = nb_cdiv(p, NB_MP_TILE);
    NB_REQUIRE((long long)n * tiles * tiles <= 0x7fffffffll, "metric_pairs: n %d pairs of %d x %d tiles exceed the grid", n, tiles, tiles);
    if (n == 0) return NB_OK;
    const bool vec = (p & 3) == 0 && (r & 3) == 0 && (stride_n & 3) == 0 && (((uintptr_t)renders | (uintptr_t)blur1 | (uintptr_t)out) & 15) == 0;
    MpParams P{renders, stride_n, blur1, mean, off0, off1, src1, k, r, p, n, tiles, masked ? 1 : 0, out};
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((long long)n * tiles * tiles)), block(NB_MP_THREADS);
    if (vec && tr) hipLaunchKernelGGL((metric_pairs_kernel<4, true>), grid, block, 0, st, P);
    else if (vec) hipLaunchKernelGGL((metric_pairs_kernel<4, false>), grid, block, 0, st, P);
    else if (tr) hipLaunchKernelGGL((metric_pairs_kernel<1, true>), grid, block, 0, st, P);
    else hipLaunchKernelGGL((metric_pairs_kernel<1, false>), grid, block, 0, st, P);
    NB_CHECK_LAUNCH("metric_pairs");
    return NB_OK;
}
