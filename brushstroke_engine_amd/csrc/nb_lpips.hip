// The LPIPS network for gfx950 (perceptual.LPIPS): everything around the trunk's convolutions, which run on the project's conv kernels.
//
//   nb_lpips_scale_f32           the scaling layer, y = (x - shift_c) / scale_c; its backward is the same launch without a shift.
//   nb_lpips_relu_pool_f32       from a convolution's raw output and a per-channel bias: the tap map max(x + b, 0) and, if a pool
//                                follows, the pooled map (windows of 2 or 3, stride 2, floor mode, no padding), in one launch.
//   nb_lpips_relu_pool_bwd_f32   the gradient of the raw output from d_tap and / or d_pooled, one thread per element, gathering: the
//                                pool's gradient goes to the FIRST maximum of a window in row-major order, nothing flows where the tap is 0.
//   nb_lpips_head_f32            per level: the five channel sums of a pixel (sum f0^2, sum f1^2, sum w f0^2, sum w f1^2, sum w f0 f1)
//                                in ONE pass over the channels, from them d = sum_c w_c (u0_c - u1_c)^2 and the values the backward
//                                keeps, per-sample partial sums, and a finishing launch that adds the level's mean into acc [n].
//   nb_lpips_head_bwd_f32        the gradient of f1 from the kept values and an upstream [n].
//
// Data is fp32, NCHW, dense.  The five channel sums of the head, and the combination P i0^2 + Q i1^2 - 2 X i0 i1 that follows, are carried
// in fp64 registers: the expanded form cancels where the two images are alike, and the kernel is bound by its loads.  Everything that
// is stored is fp32.  No float atomics: sums are lanes by halving, waves one after the other, workgroups one after the other, so the
// same input gives the same bits and sample i of an n-sample call equals the one-sample call on it (the form of the head kernel is
// chosen from c and h * w alone).
#include "nb_common.h"
#include <cstdint>

#define LP_THREADS 256
#define LP_SPLIT_PIX 16                                                    // channel-split head: 16 pixels x 16 channel slices per workgroup
#define LP_SPLIT_SLICES 16
#define LP_EPS 1e-10

static inline bool lp_split_form(int c, int hw) { return hw <= NB_LPIPS_SPLIT_MAX_HW && c >= NB_LPIPS_SPLIT_MIN_C; }
static inline int lp_parts(int c, int hw) { return lp_split_form(c, hw) ? nb_cdiv(hw, LP_SPLIT_PIX) : nb_cdiv(hw, LP_THREADS); }

extern "C" long long nb_lpips_head_parts(int c, int hw) {
    if (c < 1 || hw < 1) { nb_set_error("lpips_head_parts: bad sizes (c %d, hw %d)", c, hw); return -1; }
    return lp_parts(c, hw);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// scaling layer
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LP_THREADS) void lpips_scale_kernel(const float* __restrict__ x, const float* __restrict__ shift,
                                                                 const float* __restrict__ scale, float* __restrict__ y, int c, long long hw,
                                                                 long long total) {
    const long long e = (long long)blockIdx.x * LP_THREADS + threadIdx.x;
    if (e >= total) return;
    const int ch = (int)((e / hw) % c);
    const float v = x[e] - (shift ? shift[ch] : 0.f);
    y[e] = v / scale[ch];
}

extern "C" int nb_lpips_scale_f32(const float* x, const float* shift, const float* scale, float* y, int n, int c, long long hw, void* stream) {
    NB_REQUIRE(x && scale && y, "lpips_scale: null pointer");
    NB_REQUIRE(n >= 0 && c >= 1 && hw >= 1 && (long long)n * c * hw <= (1ll << 38), "lpips_scale: bad sizes (n %d, c %d, hw %lld)", n, c, hw);
    NB_REQUIRE((((uintptr_t)x | (uintptr_t)shift | (uintptr_t)scale | (uintptr_t)y) & 3) == 0, "lpips_scale: the float pointers must be 4-byte aligned");
    const long long total = (long long)n * c * hw;
    if (total == 0) return NB_OK;
    hipLaunchKernelGGL(lpips_scale_kernel, dim3((unsigned)((total + LP_THREADS - 1) / LP_THREADS)), dim3(LP_THREADS), 0, (hipStream_t)stream, x, shift,
                       scale, y, c, hw, total);
    NB_CHECK_LAUNCH("lpips_scale");
    return NB_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// bias + ReLU + tap + max-pool
// ---------------------------------------------------------------------------------------------------------------------------------
struct LpPool { int c, h, w, win, ph, pw; long long per_sample; };

static int lp_pool_sizes(const char* what, int n, int c, int h, int w, int win, LpPool& P) {
    NB_REQUIRE(n >= 0 && n <= 65535 && c >= 1 && h >= 1 && w >= 1 && (long long)c * h * w < (1ll << 31),
               "%s: bad sizes (n %d in 0..65535, c %d, h %d, w %d, c * h * w below 2^31)", what, n, c, h, w);
    NB_REQUIRE(win == 0 || ((win == 2 || win == 3) && h >= win && w >= win), "%s: window %d on %d x %d: 0 (no pool), 2 or 3, not above the map", what,
               win, h, w);
    P.c = c; P.h = h; P.w = w; P.win = win;
    P.ph = win ? (h - win) / 2 + 1 : 0;
    P.pw = win ? (w - win) / 2 + 1 : 0;
    P.per_sample = (long long)c * h * w;
    return NB_OK;
}

__global__ __launch_bounds__(LP_THREADS) void lpips_relu_pool_kernel(LpPool P, const float* __restrict__ x, const float* __restrict__ bias,
                                                                     float* __restrict__ tap, float* __restrict__ pooled) {
    const long long e = (long long)blockIdx.x * LP_THREADS + threadIdx.x;
    if (e >= P.per_sample) return;
    const int n = blockIdx.y, hw = P.h * P.w;
    const int ch = (int)(e / hw), pix = (int)(e - (long long)ch * hw), yy = pix / P.w, xx = pix - yy * P.w;
    const float b = bias[ch];
    const float* xs = x + (long long)n * P.per_sample + (long long)ch * hw;
    const float v = fmaxf(xs[pix] + b, 0.f);
    tap[(long long)n * P.per_sample + e] = v;
    // the thread of a window's first pixel also writes the pooled value (the window's other raw values come from the cache)
    if (P.win && !(yy & 1) && !(xx & 1) && (yy >> 1) < P.ph && (xx >> 1) < P.pw) {
        float m = v;
        for (int a = 0; a < P.win; ++a)
            for (int q = 0; q < P.win; ++q) m = fmaxf(m, fmaxf(xs[(yy + a) * P.w + xx + q] + b, 0.f));
        pooled[((long long)n * P.c + ch) * P.ph * P.pw + (yy >> 1) * P.pw + (xx >> 1)] = m;
    }
}

extern "C" int nb_lpips_relu_pool_f32(const float* x, const float* bias, float* tap, float* pooled, int n, int c, int h, int w, int window,
                                      void* stream) {
    NB_REQUIRE(x && bias && tap && (pooled || window == 0), "lpips_relu_pool: null pointer");
    LpPool P;
    if (lp_pool_sizes("lpips_relu_pool", n, c, h, w, window, P) != NB_OK) return NB_EINVAL;
    NB_REQUIRE((((uintptr_t)x | (uintptr_t)bias | (uintptr_t)tap | (uintptr_t)pooled) & 3) == 0, "lpips_relu_pool: the float pointers must be 4-byte aligned");
    if (n == 0) return NB_OK;
    hipLaunchKernelGGL(lpips_relu_pool_kernel, dim3((unsigned)((P.per_sample + LP_THREADS - 1) / LP_THREADS), n), dim3(LP_THREADS), 0,
                       (hipStream_t)stream, P, x, bias, tap, pooled);
    NB_CHECK_LAUNCH("lpips_relu_pool");
    return NB_OK;
}

__global__ __launch_bounds__(LP_THREADS) void lpips_relu_pool_bwd_kernel(LpPool P, const float* __restrict__ tap, const float* __restrict__ d_tap,
                                                                         const float* __restrict__ d_pooled, float* __restrict__ d_x) {
    const long long e = (long long)blockIdx.x * LP_THREADS + threadIdx.x;
    if (e >= P.per_sample) return;
    const int n = blockIdx.y, hw = P.h * P.w;
    const int ch = (int)(e / hw), pix = (int)(e - (long long)ch * hw), yy = pix / P.w, xx = pix - yy * P.w;
    const float* ts = tap + (long long)n * P.per_sample + (long long)ch * hw;
    const float v = ts[pix];
    float g = 0.f;
    if (v != 0.f) {                                                        // (v > 0: the tap is a ReLU output)
        if (d_tap) g = d_tap[(long long)n * P.per_sample + e];
        if (d_pooled) {
            const float* dp = d_pooled + ((long long)n * P.c + ch) * P.ph * P.pw;
            const int py0 = max(0, (yy - P.win + 2) / 2), py1 = min(P.ph - 1, yy >> 1);
            const int px0 = max(0, (xx - P.win + 2) / 2), px1 = min(P.pw - 1, xx >> 1);
            for (int py = py0; py <= py1; ++py)
                for (int px = px0; px <= px1; ++px) {
                    // is (yy, xx) the first maximum of window (py, px)?  earlier pixels must be below v, later ones not above it
                    bool first = true;
                    for (int a = 0; a < P.win; ++a)
                        for (int q = 0; q < P.win; ++q) {
                            const int wy = 2 * py + a, wx = 2 * px + q;
                            const float t = ts[wy * P.w + wx];
                            const bool earlier = wy < yy || (wy == yy && wx < xx);
                            if (earlier ? t >= v : t > v) first = false;
                        }
                    if (first) g += dp[py * P.pw + px];
                }
        }
    }
    d_x[(long long)n * P.per_sample + e] = g;
}

extern "C" int nb_lpips_relu_pool_bwd_f32(const float* tap, const float* d_tap, const float* d_pooled, float* d_x, int n, int c, int h, int w,
                                          int window, void* stream) {
    NB_REQUIRE(tap && d_x, "lpips_relu_pool_bwd: null pointer");
    NB_REQUIRE(d_pooled == nullptr || window != 0, "lpips_relu_pool_bwd: d_pooled without a pool");
    LpPool P;
    if (lp_pool_sizes("lpips_relu_pool_bwd", n, c, h, w, window, P) != NB_OK) return NB_EINVAL;
    NB_REQUIRE((((uintptr_t)tap | (uintptr_t)d_tap | (uintptr_t)d_pooled | (uintptr_t)d_x) & 3) == 0,
               "lpips_relu_pool_bwd: the float pointers must be 4-byte aligned");
    if (n == 0) return NB_OK;
    hipLaunchKernelGGL(lpips_relu_pool_bwd_kernel, dim3((unsigned)((P.per_sample + LP_THREADS - 1) / LP_THREADS), n), dim3(LP_THREADS), 0,
                       (hipStream_t)stream, P, tap, d_tap, d_pooled, d_x);
    NB_CHECK_LAUNCH("lpips_relu_pool_bwd");
    return NB_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// head
// ---------------------------------------------------------------------------------------------------------------------------------
struct LpHead {
    const float* f0; const float* f1; const float* w;
    int c, hw, parts;
    long long n_hw;                                                        // n * hw: the pitch of the three kept planes
    float* kept; float* partials;
};

struct LpSums { double a, b, p, q, x; };

__device__ __forceinline__ void lp_accumulate(LpSums& s, float x0, float x1, float wc) {
    const double d0 = (double)x0, d1 = (double)x1, dw = (double)wc;
    s.a += d0 * d0;
    s.b += d1 * d1;
    s.p += dw * (d0 * d0);
    s.q += dw * (d1 * d1);
    s.x += dw * (d0 * d1);
}

// d of a pixel from its five sums; kept[0] = 1 / (|f0| + eps) (0 where f0 = 0), kept[1] = |f1|, kept[2] = sum_c w_c e_c f1_c
__device__ __forceinline__ float lp_pixel(const LpSums& s, float* kept, long long n_hw, long long at) {
    const double s1 = sqrt(s.b);
    const double i0 = s.a > 0.0 ? 1.0 / (sqrt(s.a) + LP_EPS) : 0.0, i1 = s.b > 0.0 ? 1.0 / (s1 + LP_EPS) : 0.0;
    kept[at] = (float)i0;
    kept[n_hw + at] = (float)s1;
    kept[2 * n_hw + at] = (float)(s.q * i1 - s.x * i0);
    return (float)((s.p * i0 * i0 + s.q * i1 * i1) - 2.0 * s.x * i0 * i1);
}

__device__ __forceinline__ float lp_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_down(v, o);
    return v;
}

// one thread per pixel walks the channels (coalesced over the pixels); a workgroup leaves the sum of its 256 pixels
__global__ __launch_bounds__(LP_THREADS) void lpips_head_pixel_kernel(LpHead p) {
    __shared__ float wsum[LP_THREADS / 64];
    const int tid = threadIdx.x, n = blockIdx.y, pix = blockIdx.x * LP_THREADS + tid;
    float d = 0.f;
    if (pix < p.hw) {
        const float* a = p.f0 + (long long)n * p.c * p.hw + pix;
        const float* b = p.f1 + (long long)n * p.c * p.hw + pix;
        LpSums s{0.0, 0.0, 0.0, 0.0, 0.0};
        for (int ch = 0; ch < p.c; ++ch) lp_accumulate(s, a[(long long)ch * p.hw], b[(long long)ch * p.hw], p.w[ch]);
        d = lp_pixel(s, p.kept, p.n_hw, (long long)n * p.hw + pix);
    }
    d = lp_wave_sum(d);
    if ((tid & 63) == 0) wsum[tid >> 6] = d;
    __syncthreads();
    if (tid == 0) {
        float r = wsum[0];
        for (int wv = 1; wv < LP_THREADS / 64; ++wv) r += wsum[wv];
        p.partials[(long long)n * p.parts + blockIdx.x] = r;
    }
}

// small maps with many channels: 16 pixels x 16 channel slices per workgroup, slice s takes channels s, s + 16, ...; the slices' sums
// meet in LDS and are added in their order
__global__ __launch_bounds__(LP_THREADS) void lpips_head_split_kernel(LpHead p) {
    __shared__ double sums[LP_SPLIT_SLICES][LP_SPLIT_PIX][5];
    __shared__ float dpix[LP_SPLIT_PIX];
    const int tid = threadIdx.x, n = blockIdx.y, lp = tid & (LP_SPLIT_PIX - 1), sl = tid / LP_SPLIT_PIX;
    const int pix = blockIdx.x * LP_SPLIT_PIX + lp;
    LpSums s{0.0, 0.0, 0.0, 0.0, 0.0};
    if (pix < p.hw) {
        const float* a = p.f0 + (long long)n * p.c * p.hw + pix;
        const float* b = p.f1 + (long long)n * p.c * p.hw + pix;
        for (int ch = sl; ch < p.c; ch += LP_SPLIT_SLICES) lp_accumulate(s, a[(long long)ch * p.hw], b[(long long)ch * p.hw], p.w[ch]);
    }
    double* mine = sums[sl][lp];
    mine[0] = s.a; mine[1] = s.b; mine[2] = s.p; mine[3] = s.q; mine[4] = s.x;
    __syncthreads();
    if (tid < LP_SPLIT_PIX) {
        float d = 0.f;
        if (pix < p.hw) {
            LpSums t{0.0, 0.0, 0.0, 0.0, 0.0};
            for (int q = 0; q < LP_SPLIT_SLICES; ++q) {
                const double* o = sums[q][tid];
                t.a += o[0]; t.b += o[1]; t.p += o[2]; t.q += o[3]; t.x += o[4];
            }
            d = lp_pixel(t, p.kept, p.n_hw, (long long)n * p.hw + pix);
        }
        dpix[tid] = d;
    }
    __syncthreads();
    if (tid == 0) {
        float r = dpix[0];
        for (int q = 1; q < LP_SPLIT_PIX; ++q) r += dpix[q];
        p.partials[(long long)n * p.parts + blockIdx.x] = r;
    }
}

__global__ __launch_bounds__(LP_THREADS) void lpips_head_finish_kernel(const float* __restrict__ partials, int n, int parts, int hw, float* __restrict__ acc) {
    const int i = blockIdx.x * LP_THREADS + threadIdx.x;
    if (i >= n) return;
    const float* q = partials + (long long)i * parts;
    float s = q[0];
    for (int k = 1; k < parts; ++k) s += q[k];
    acc[i] += s / (float)hw;
}

static int lp_head_sizes(const char* what, int n, int c, int hw) {
    NB_REQUIRE(n >= 0 && n <= 65535 && c >= 1 && hw >= 1 && (long long)c * hw < (1ll << 31),
               "%s: bad sizes (n %d in 0..65535, c %d, hw %d, c * hw below 2^31)", what, n, c, hw);
    return NB_OK;
}

extern "C" int nb_lpips_head_f32(const float* f0, const float* f1, const float* w, int n, int c, int hw, float* kept, float* partials, float* acc,
                                 void* stream) {
    NB_REQUIRE(f0 && f1 && w && kept && partials && acc, "lpips_head: null pointer");
    if (lp_head_sizes("lpips_head", n, c, hw) != NB_OK) return NB_EINVAL;
    NB_REQUIRE((((uintptr_t)f0 | (uintptr_t)f1 | (uintptr_t)w | (uintptr_t)kept | (uintptr_t)partials | (uintptr_t)acc) & 3) == 0,
               "lpips_head: the float pointers must be 4-byte aligned");
    if (n == 0) return NB_OK;
    hipStream_t st = (hipStream_t)stream;
    LpHead p{f0, f1, w, c, hw, lp_parts(c, hw), (long long)n * hw, kept, partials};
    if (lp_split_form(c, hw)) hipLaunchKernelGGL(lpips_head_split_kernel, dim3(p.parts, n), dim3(LP_THREADS), 0, st, p);
    else hipLaunchKernelGGL(lpips_head_pixel_kernel, dim3(p.parts, n), dim3(LP_THREADS), 0, st, p);
    NB_CHECK_LAUNCH("lpips_head");
    hipLaunchKernelGGL(lpips_head_finish_kernel, dim3(nb_cdiv(n, LP_THREADS)), dim3(LP_THREADS), 0, st, (const float*)partials, n, p.parts, hw, acc);
    NB_CHECK_LAUNCH("lpips_head_finish");
    return NB_OK;
}

struct LpHeadBwd {
    const float* f0; const float* f1; const float* w; const float* kept; const float* g;
    int c, hw, accumulate;
    long long n_hw;
    float* d_f1;
};

__global__ __launch_bounds__(LP_THREADS) void lpips_head_bwd_kernel(LpHeadBwd p) {
    const long long e = (long long)blockIdx.x * LP_THREADS + threadIdx.x, per = (long long)p.c * p.hw;
    if (e >= per) return;
    const int n = blockIdx.y, ch = (int)(e / p.hw), pix = (int)(e - (long long)ch * p.hw);
    const long long at = (long long)n * p.hw + pix, idx = (long long)n * per + e;
    const float i0 = p.kept[at], s1 = p.kept[p.n_hw + at], q = p.kept[2 * p.n_hw + at];
    float r = 0.f;
    if (s1 > 0.f) {
        const float n1 = s1 + (float)LP_EPS, x1 = p.f1[idx], wc = p.w[ch];
        const float ek = x1 / n1 - p.f0[idx] * i0;
        const float up = p.g[n] / (float)p.hw;
        r = up * ((2.f * wc * ek) / n1 - x1 * ((2.f * q) / ((n1 * n1) * s1)));
    }
    p.d_f1[idx] = p.accumulate ? p.d_f1[idx] + r : r;
}

extern "C" int nb_lpips_head_bwd_f32(const float* f0, const float* f1, const float* w, const float* kept, const float* g, int n, int c, int hw,
                                     int accumulate, float* d_f1, void* stream) {
    NB_REQUIRE(f0 && f1 && w && kept && g && d_f1, "lpips_head_bwd: null pointer");
    if (lp_head_sizes("lpips_head_bwd", n, c, hw) != NB_OK) return NB_EINVAL;
    NB_REQUIRE((((uintptr_t)f0 | (uintptr_t)f1 | (uintptr_t)w | (uintptr_t)kept | (uintptr_t)g | (uintptr_t)d_f1) & 3) == 0,
               "lpips_head_bwd: the float pointers must be 4-byte aligned");
    if (n == 0) return NB_OK;
    LpHeadBwd p{f0, f1, w, kept, g, c, hw, accumulate != 0, (long long)n * hw, d_f1};
    const long long per = (long long)c * hw;
    hipLaunchKernelGGL(lpips_head_bwd_kernel, dim3((unsigned)((per + LP_THREADS - 1) / LP_THREADS), n), dim3(LP_THREADS), 0, (hipStream_t)stream, p);
    NB_CHECK_LAUNCH("lpips_head_bwd");
    return NB_OK;
}
