// Inputs of the stitching scores for gfx950 (metrics.BrushEvaluator with a StitchSetup): what the reference's metric loop
// (forger/metrics/metric_main.py:181-200) and compute_stitching_metrics (forger/metrics/geom_metric.py:165-187) do around the two
// generator passes of RandomStitcher.generate_with_stitching (forger/train/stitching.py:212-267) -- two crops of every full-size
// drawing before them; the mask, the multiply, the slice-add of CropHelper.composite (stitching.py:161-179), the margin crop and
// the L1 in each direction behind them: a loop of copies and about twenty small torch launches per (brush, round) there, two
// launches (and a finish) per generator pass here.
//
// nb_stitch_crops_u8 gathers the R x R windows of the full drawings [K,D,D] uint8 as the generator's geometry input [n,1,R,R]
// float32, value / 255 in correctly rounded fp32 (the quotient is taken in fp64 and rounded once more: no double of the form
// v / 255, v an integer in 0..255, lies within 2^-53 relative of a midpoint of two floats, so the result is the correctly rounded
// one; tests/stitch_refs.py checks the 256 values).  Every unit has its own window pair, so n windows go in one launch.
//
// nb_stitch_pairs_f32 is the hot path, one launch per pass.  It reads the raw generator images fake [2n,3,R,R] (rows :n the first
// crops, rows n: the second) and writes the LPIPS input of 2n pairs, out [4n,3,S,S]: the two images cropped, and each with the
// other's pixels composited into it, cropped likewise.  The crop is img[:, :, margin:R - 2 margin, margin:R - 2 margin]
// (geom_metric.py:173-177): `margin` is taken off the top and left and TWICE `margin` off the bottom and right, so S = R - 3 margin.
// It is asymmetric (the symmetric crop would be R - 2 margin wide); the reference's numbers are defined by it, so it is kept.
// Every value written is a copy of an input float: the images go to the network unscaled, as the reference hands raw `fake` to it.
// The same pass sums |first - second| of both pairs of a sample: NB_STITCH_PARTS workgroups share a sample and leave two partial
// sums each; a small second launch adds a pair's partials in their order.  Lanes reduce by halving, waves one after the other: no
// float atomics, the same input gives the same bits.
//
// A work item is G consecutive output columns of one row of one colour plane.  With S, R, margin and the sample stride multiples of
// four and fake and out 16-byte aligned, G = 4: a thread loads both images' quads and stores four quads as 16-byte vectors; the
// composite's source is shifted by the difference of the two rectangles' corners, which is any number of columns, so those loads are
// 4 bytes each (they touch the overlap only).  Otherwise (S = 226 at R = 256 and margin 10; odd S; a misaligned base) G = 1 and 64
// lanes move a 256-byte row segment per request.
//
// The rectangles live on the device and cannot be checked on the host: the kernel treats a rectangle pair that is empty, leaves the
// image or whose two extents differ as "no composite" (the second side equals the first, the sum is 0), and the crop kernel clamps a
// drawing index into 0..K - 1 and a window into 0..D - R, so a bad plan gives a wrong picture, never an access outside the buffers.
#include "nb_common.h"
#include <cstdint>

#define NB_ST_THREADS 256
#define NB_ST_PARTS NB_STITCH_PARTS

// ---- the crops ----
struct ScParams {
    const uint8_t* drawings; const int32_t* draw; const int32_t* off;
    int k, d, r, n, blocks;
    float* out;
};

template <int G>
__global__ __launch_bounds__(NB_ST_THREADS) void stitch_crops_kernel(ScParams P) {
    const int i = blockIdx.x / P.blocks, b = blockIdx.x % P.blocks, r = P.r, d = P.d;
    const int gpr = r / G;                                                 // (G == 4 only when r is a multiple of four)
    const int g = b * NB_ST_THREADS + threadIdx.x;
    if (g >= r * gpr) return;
    const int y = g / gpr, x = (g % gpr) * G;
    const int j = min(max(P.draw[i], 0), P.k - 1);
    const int oy = min(max(P.off[2 * i], 0), d - r), ox = min(max(P.off[2 * i + 1], 0), d - r);
    const uint8_t* src = P.drawings + (size_t)j * d * d + (size_t)(oy + y) * d + (size_t)(ox + x);
    float* dst = P.out + (size_t)i * r * r + (size_t)y * r + x;
    float v[G];
#pragma unroll
    for (int q = 0; q < G; ++q) v[q] = (float)((double)src[q] / 255.0);
    if (G == 4) *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1 % G], v[2 % G], v[3 % G]);
    else dst[0] = v[0];
}

extern "C" int nb_stitch_crops_u8(const uint8_t* drawings, int k, int d, const int32_t* draw, const int32_t* off, int n, int r, float* out,
                                  void* stream) {
    NB_REQUIRE(drawings && draw && off && out, "stitch_crops: null pointer");
    NB_REQUIRE(k >= 1 && k <= 65535 && r >= 1 && r <= 8192 && d >= r && d <= 32768 && n >= 0 && n <= (1 << 24),
               "stitch_crops: bad sizes (k %d outside 1..65535, r %d outside 1..8192, d %d outside r..32768, n %d outside 0..2^24)", k, r, d, n);
    NB_REQUIRE((((uintptr_t)draw | (uintptr_t)off | (uintptr_t)out) & 3) == 0, "stitch_crops: draw, off and out must be 4-byte aligned");
    const bool vec = (r & 3) == 0 && ((uintptr_t)out & 15) == 0;
    const int blocks = nb_cdiv(vec ? r * (r / 4) : r * r, NB_ST_THREADS);
    NB_REQUIRE((long long)n * blocks <= 0x7fffffffll, "stitch_crops: n %d windows of %d workgroups exceed the grid", n, blocks);
    if (n == 0) return NB_OK;
    ScParams P{drawings, draw, off, k, d, r, n, blocks, out};
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((long long)n * blocks)), block(NB_ST_THREADS);
    if (vec) hipLaunchKernelGGL(stitch_crops_kernel<4>, grid, block, 0, st, P);
    else hipLaunchKernelGGL(stitch_crops_kernel<1>, grid, block, 0, st, P);
    NB_CHECK_LAUNCH("stitch_crops");
    return NB_OK;
}

// ---- the pairs ----
struct SpParams {
    const float* fake; long long stride_n;
    const int32_t* rects_a; const int32_t* rects_b;
    int r, s, margin, n, gpr, total, per_part;
    float* out; float* partials;
};

// where a composite writes (rows r0..r1, columns c0..c1 of the destination image) and how far its source lies from there
struct StRect { int r0, c0, r1, c1, dr, dc; };

// dst / src: (rstart, cstart, rend, cend) each.  Empty, outside the image or of different extents: nothing is composited.
__device__ __forceinline__ StRect st_rect(const int32_t* dst, const int32_t* src, int r) {
    StRect q{dst[0], dst[1], dst[2], dst[3], 0, 0};
    const int sr0 = src[0], sc0 = src[1], sr1 = src[2], sc1 = src[3];
    const bool ok = q.r0 >= 0 && q.r0 < q.r1 && q.r1 <= r && q.c0 >= 0 && q.c0 < q.c1 && q.c1 <= r &&
                    sr0 >= 0 && sr1 <= r && sc0 >= 0 && sc1 <= r && sr1 - sr0 == q.r1 - q.r0 && sc1 - sc0 == q.c1 - q.c0;
    if (!ok) { q.r0 = q.r1 = q.c0 = q.c1 = 0; return q; }
    q.dr = sr0 - q.r0; q.dc = sc0 - q.c0;
    return q;
}

template <int G>
__device__ __forceinline__ void st_load(const float* q, float (&v)[G]) {
    if (G == 4) {
        const float4 f = *reinterpret_cast<const float4*>(q);
        v[0] = f.x; v[1 % G] = f.y; v[2 % G] = f.z; v[3 % G] = f.w;
    } else {
        v[0] = q[0];
    }
}

template <int G>
__device__ __forceinline__ void st_store(float* q, const float (&v)[G]) {
    if (G == 4) *reinterpret_cast<float4*>(q) = make_float4(v[0], v[1 % G], v[2 % G], v[3 % G]);
    else q[0] = v[0];
}

template <int G>
__global__ __launch_bounds__(NB_ST_THREADS) void stitch_pairs_kernel(SpParams P) {
    __shared__ float wsum[NB_ST_THREADS / 64][2];
    const int tid = threadIdx.x, i = blockIdx.x / NB_ST_PARTS, part = blockIdx.x % NB_ST_PARTS;
    const int r = P.r, s = P.s, m = P.margin, gpr = P.gpr;
    const size_t count = (size_t)r * r, scount = (size_t)s * s;
    const float* f1 = P.fake + (long long)i * P.stride_n;
    const float* f2 = P.fake + ((long long)P.n + i) * P.stride_n;
    // first pair: fake2's area2 into fake1's area1; second pair: fake1's area1 into fake2's area2 (stitching.py:248-253)
    const StRect A = st_rect(P.rects_a + 8 * i, P.rects_a + 8 * i + 4, r);
    const StRect B = st_rect(P.rects_b + 8 * i + 4, P.rects_b + 8 * i, r);
    float* o0 = P.out + (size_t)i * 3 * scount;
    float* o1 = P.out + ((size_t)P.n + i) * 3 * scount;
    float* o2 = P.out + (2 * (size_t)P.n + i) * 3 * scount;
    float* o3 = P.out + (3 * (size_t)P.n + i) * 3 * scount;
    const int g0 = part * P.per_part, g1 = min(P.total, g0 + P.per_part);
    float sa = 0.f, sb = 0.f;
    for (int g = g0 + tid; g < g1; g += NB_ST_THREADS) {
        const int c = g / (s * gpr), rem = g % (s * gpr), y = rem / gpr, x = (rem % gpr) * G;
        const int yy = y + m, xx = x + m;                                  // the pixel in the images
        const size_t o = (size_t)c * count + (size_t)yy * r + xx;
        float v1[G], v2[G], a[G], b[G];
        st_load<G>(f1 + o, v1);
        st_load<G>(f2 + o, v2);
        const bool rowa = yy >= A.r0 && yy < A.r1, rowb = yy >= B.r0 && yy < B.r1;
#pragma unroll
        for (int q = 0; q < G; ++q) {
            a[q] = v1[q];
            b[q] = v2[q];
            if (rowa && xx + q >= A.c0 && xx + q < A.c1) {
                a[q] = f2[(size_t)c * count + (size_t)(yy + A.dr) * r + (size_t)(xx + q + A.dc)];
                sa += fabsf(v1[q] - a[q]);
            }
            if (rowb && xx + q >= B.c0 && xx + q < B.c1) {
                b[q] = f1[(size_t)c * count + (size_t)(yy + B.dr) * r + (size_t)(xx + q + B.dc)];
                sb += fabsf(v2[q] - b[q]);
            }
        }
        const size_t po = (size_t)c * scount + (size_t)y * s + x;
        st_store<G>(o0 + po, v1);
        st_store<G>(o1 + po, v2);
        st_store<G>(o2 + po, a);
        st_store<G>(o3 + po, b);
    }
    // fixed-order reduce: lanes by halving, then the waves one after the other
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        sa += __shfl_down(sa, o);
        sb += __shfl_down(sb, o);
    }
    if ((tid & 63) == 0) {
        wsum[tid >> 6][0] = sa;
        wsum[tid >> 6][1] = sb;
    }
    __syncthreads();
    if (tid < 2) {
        float t = wsum[0][tid];
        for (int w = 1; w < NB_ST_THREADS / 64; ++w) t += wsum[w][tid];
        P.partials[((size_t)i * NB_ST_PARTS + part) * 2 + tid] = t;
    }
}

__global__ __launch_bounds__(256) void stitch_l1_finish_kernel(const float* __restrict__ partials, int n, float* __restrict__ l1) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= 2 * n) return;
    const int i = t % n, which = t / n;                                    // l1[:n] the first pairs, l1[n:] the second
    float s = partials[((size_t)i * NB_ST_PARTS) * 2 + which];
    for (int b = 1; b < NB_ST_PARTS; ++b) s += partials[((size_t)i * NB_ST_PARTS + b) * 2 + which];
    l1[t] = s;
}

extern "C" int nb_stitch_pairs_f32(const float* fake, long long stride_n, const int32_t* rects_a, const int32_t* rects_b, int n, int r, int margin,
                                   float* out, float* l1, float* partials, void* stream) {
    NB_REQUIRE(fake && rects_a && rects_b && out && l1 && partials, "stitch_pairs: null pointer");
    NB_REQUIRE(r >= 1 && r <= 8192 && n >= 0 && n <= (1 << 22), "stitch_pairs: bad sizes (r %d outside 1..8192, n %d outside 0..2^22)", r, n);
    NB_REQUIRE(margin >= 0 && 3ll * margin < r, "stitch_pairs: margin %d leaves no crop window of r = %d (r - 3 * margin must be at least 1)", margin, r);
    const long long count = (long long)r * r;
    NB_REQUIRE(stride_n >= 3 * count, "stitch_pairs: stride_n %lld below 3 * r * r = %lld: the images would alias", stride_n, 3 * count);
    NB_REQUIRE((((uintptr_t)fake | (uintptr_t)rects_a | (uintptr_t)rects_b | (uintptr_t)out | (uintptr_t)l1 | (uintptr_t)partials) & 3) == 0,
               "stitch_pairs: the float and int pointers must be 4-byte aligned");
    if (n == 0) return NB_OK;
    const int s = r - 3 * margin;
    const bool vec = (s & 3) == 0 && (r & 3) == 0 && (margin & 3) == 0 && (stride_n & 3) == 0 && (((uintptr_t)fake | (uintptr_t)out) & 15) == 0;
    const int gpr = vec ? s / 4 : s;
    const int total = 3 * s * gpr;                                         // (at most 3 * 8192^2 < 2^31)
    SpParams P{fake, stride_n, rects_a, rects_b, r, s, margin, n, gpr, total, nb_cdiv(total, NB_ST_PARTS), out, partials};
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)(n * NB_ST_PARTS)), block(NB_ST_THREADS);
    if (vec) hipLaunchKernelGGL(stitch_pairs_kernel<4>, grid, block, 0, st, P);
    else hipLaunchKernelGGL(stitch_pairs_kernel<1>, grid, block, 0, st, P);
    NB_CHECK_LAUNCH("stitch_pairs");
    hipLaunchKernelGGL(stitch_l1_finish_kernel, dim3(nb_cdiv(2 * n, 256)), dim3(256), 0, st, (const float*)partials, n, l1);
    NB_CHECK_LAUNCH("stitch_pairs_finish");
    return NB_OK;
}
