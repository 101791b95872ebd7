// Brush projection for gfx950 (projection.BrushProjector): the loss that the reference's project() (scripts/project_main.py:38-224)
// computes around the generator, for k exemplars of b patches each (sample n = exemplar * b + patch; every exemplar has its own
// drawings).  The regulariser, Adam and the per-plane renormalisation of project() (:115, 172-181, 209-218) are nb_noise_reg_f32 and
// nb_clarity_step_f32 of nb_clarity.hip.
//
//   nb_projection_masks_f32     once per pass: the conservative masks of get_conservative_fg_bg (forger/metrics/geom_metric.py:132-140)
//                               from the twice-blurred drawings, their counts per exemplar and the exemplar's mean background colour
//                               (compute_masked_color, project_main.py:248-250).
//   nb_projection_loss_f32      the composite over the background colour or image (composite_with_bg_color / composite_with_bg_image,
//                               project_main.py:227-245, with compose_stroke of forger/viz/visualize.py:315-323), the L1 over the
//                               foreground (:164-165) and the background item over uvs[2] (:167-168).
//   nb_projection_loss_bwd_f32  their gradient with respect to uvs, colors (composite) or the image (no composite), with an optional
//                               upstream gradient of the composite (the perceptual item's).
//
// NB_PROJECTION_PARTS workgroups share a sample and leave partial sums, a small second launch adds them in their order.  fp32
// throughout, no float atomics: every sum is lanes by halving, waves one after the other, parts one after the other, patches one
// after the other, so the same input gives the same bits and row i of a k-row call equals the one-row call on that row.  Planes are
// read in 16-byte vectors when r * r and the strides are multiples of four and the bases are 16-byte aligned, else pixel by pixel.
#include "nb_common.h"
#include <cstdint>

#define PJ_THREADS 256
#define PJ_PARTS NB_PROJECTION_PARTS

template <int VEC> struct PjIo;
template <> struct PjIo<1> {
    static __device__ __forceinline__ void load(const float* p, float* v) { v[0] = *p; }
    static __device__ __forceinline__ void store(float* p, const float* v) { *p = v[0]; }
    static __device__ __forceinline__ uint32_t load_mask(const uint8_t* p) { return *p; }
    static __device__ __forceinline__ void store_mask(uint8_t* p, uint32_t m) { *p = (uint8_t)m; }
};
template <> struct PjIo<4> {
    static __device__ __forceinline__ void load(const float* p, float* v) {
        const float4 t = *reinterpret_cast<const float4*>(p);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    }
    static __device__ __forceinline__ void store(float* p, const float* v) { *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]); }
    static __device__ __forceinline__ uint32_t load_mask(const uint8_t* p) { return *reinterpret_cast<const uint32_t*>(p); }
    static __device__ __forceinline__ void store_mask(uint8_t* p, uint32_t m) { *reinterpret_cast<uint32_t*>(p) = m; }
};

__device__ __forceinline__ float pj_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_down(v, o);
    return v;
}

// NQ sums of a workgroup, waves one after the other, to dst[0 .. NQ)
template <int NQ>
__device__ __forceinline__ void pj_block_sums(float* v, float (*wsum)[NQ], float* dst) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int q = 0; q < NQ; ++q) v[q] = pj_wave_sum(v[q]);
    if ((tid & 63) == 0) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) wsum[tid >> 6][q] = v[q];
    }
    __syncthreads();
    if (tid < NQ) {
        float s = wsum[0][tid];
        for (int w = 1; w < PJ_THREADS / 64; ++w) s += wsum[w][tid];
        dst[tid] = s;
    }
}

static int pj_sizes(const char* what, int k, int b, int r) {
    NB_REQUIRE(k >= 0 && b >= 1 && r >= 1 && r <= 4096 && (long long)k * b <= 65535,
               "%s: bad sizes (k %d, b %d, r %d; k >= 0, b >= 1, r in 1..4096, k * b <= 65535)", what, k, b, r);
    return NB_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// masks
// ---------------------------------------------------------------------------------------------------------------------------------
struct PjMaskParams {
    const float* blur; const float* target; long long target_stride;
    int count, groups_per_part;
    uint8_t* mask; float* partials;
};

// partials [n, parts, 8] = {n_fg, n_bg, sum over background of target[0], [1], [2], 0, 0, 0}; a part holds at most 2^21 pixels, so
// its counts are exact in fp32
template <int VEC>
__global__ __launch_bounds__(PJ_THREADS) void projection_masks_kernel(PjMaskParams p) {
    __shared__ float wsum[PJ_THREADS / 64][5];
    const int tid = threadIdx.x, n = blockIdx.x / PJ_PARTS, part = blockIdx.x % PJ_PARTS;
    const size_t count = (size_t)p.count;
    const float* bl = p.blur + (size_t)n * count;
    const float* tg = p.target + (long long)n * p.target_stride;
    uint8_t* md = p.mask + (size_t)n * count;
    const int ngroups = p.count / VEC;
    const int g0 = part * p.groups_per_part, g1 = min(ngroups, g0 + p.groups_per_part);
    float v[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    for (int g = g0 + tid; g < g1; g += PJ_THREADS) {
        const size_t o = (size_t)g * VEC;
        float fb[VEC], t0[VEC], t1[VEC], t2[VEC];
        PjIo<VEC>::load(bl + o, fb);
        PjIo<VEC>::load(tg + o, t0);
        PjIo<VEC>::load(tg + count + o, t1);
        PjIo<VEC>::load(tg + 2 * count + o, t2);
        uint32_t m = 0;
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            const bool bg = fb[j] >= 0.999f, fg = fb[j] < 0.1f;
            m |= ((bg ? 1u : 0u) | (fg ? 2u : 0u)) << (8 * j);
            v[0] += fg ? 1.f : 0.f;
            v[1] += bg ? 1.f : 0.f;
            v[2] += bg ? t0[j] : 0.f;
            v[3] += bg ? t1[j] : 0.f;
            v[4] += bg ? t2[j] : 0.f;
        }
        PjIo<VEC>::store_mask(md + o, m);
    }
    float* dst = p.partials + ((size_t)n * PJ_PARTS + part) * 8;
    pj_block_sums<5>(v, wsum, dst);
    if (tid >= 5 && tid < 8) dst[tid] = 0.f;
}

// one workgroup per exemplar: counts [k,2] = {n_fg, n_bg}, bg_color [k,3] = the sums over n_bg (zeros where n_bg == 0)
__global__ __launch_bounds__(64) void projection_masks_finish_kernel(const float* __restrict__ partials, int b, int32_t* __restrict__ counts,
                                                                     float* __restrict__ bg_color) {
    __shared__ int n_bg_s;
    const int tid = threadIdx.x, k = blockIdx.x;
    const float* q = partials + (size_t)k * b * PJ_PARTS * 8;
    if (tid < 2) {
        int s = 0;
        for (int i = 0; i < b * PJ_PARTS; ++i) s += (int)q[(size_t)i * 8 + tid];
        counts[2 * k + tid] = s;
        if (tid == 1) n_bg_s = s;
    }
    __syncthreads();
    if (tid < 3) {
        float s = 0.f;
        for (int i = 0; i < b * PJ_PARTS; ++i) s += q[(size_t)i * 8 + 2 + tid];
        bg_color[3 * k + tid] = n_bg_s > 0 ? s / (float)n_bg_s : 0.f;
    }
}

extern "C" int nb_projection_masks_f32(const float* blur, const float* target, long long target_stride_n, int k, int b, int r, uint8_t* mask,
                                       int32_t* counts, float* bg_color, float* partials, void* stream) {
    NB_REQUIRE(blur && target && mask && counts && bg_color && partials, "projection_masks: null pointer");
    if (pj_sizes("projection_masks", k, b, r) != NB_OK) return NB_EINVAL;
    const long long count = (long long)r * r;
    NB_REQUIRE(target_stride_n >= 3 * count, "projection_masks: the sample stride of target is below 3 * r * r = %lld: the samples would alias", 3 * count);
    NB_REQUIRE((((uintptr_t)blur | (uintptr_t)target | (uintptr_t)counts | (uintptr_t)bg_color | (uintptr_t)partials) & 3) == 0,
               "projection_masks: the float / int pointers must be 4-byte aligned");
    if (k == 0) return NB_OK;
    const bool vec = (count & 3) == 0 && (target_stride_n & 3) == 0 && (((uintptr_t)blur | (uintptr_t)target) & 15) == 0 && ((uintptr_t)mask & 3) == 0;
    const int ngroups = (int)(vec ? count / 4 : count);
    PjMaskParams p{blur, target, target_stride_n, (int)count, nb_cdiv(ngroups, PJ_PARTS), mask, partials};
    hipStream_t st = (hipStream_t)stream;
    if (vec) hipLaunchKernelGGL(projection_masks_kernel<4>, dim3(k * b * PJ_PARTS), dim3(PJ_THREADS), 0, st, p);
    else hipLaunchKernelGGL(projection_masks_kernel<1>, dim3(k * b * PJ_PARTS), dim3(PJ_THREADS), 0, st, p);
    NB_CHECK_LAUNCH("projection_masks");
    hipLaunchKernelGGL(projection_masks_finish_kernel, dim3(k), dim3(64), 0, st, (const float*)partials, b, counts, bg_color);
    NB_CHECK_LAUNCH("projection_masks_finish");
    return NB_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// loss, forward and backward
// ---------------------------------------------------------------------------------------------------------------------------------
struct PjLossParams {
    const float* uvs; long long uvs_stride;
    const float* colors;
    const float* img; long long img_stride;
    const float* target; long long target_stride;
    const float* bg_image; long long bg_stride;
    const float* bg_color;
    const uint8_t* mask; const int32_t* counts;
    const float* d_synth; const float* gscale;
    int b, count, groups_per_part;
    float w_l1, w_bg;
    float* synth; float* d_uvs; float* d_img; float* partials;
};

// the composite of one pixel and channel: stroke = sum_k uvs[k] colors[c][k] (compose_stroke), over bg with alpha = 1 - uvs[2]
__device__ __forceinline__ float pj_stroke(float u0, float u1, float u2, const float* col) { return (u0 * col[0] + u1 * col[1]) + u2 * col[2]; }
__device__ __forceinline__ float pj_synth(float stroke, float a, float bg, float u2) { return stroke * a + bg * u2; }

// the set-up the forward and the backward kernel share: pointers of sample n, its colours and its exemplar's background colour
template <int VEC, bool COMPOSITE>
struct PjSample {
    const float *u, *im, *tg, *bgi;
    const uint8_t* md;
    float col[9], bgc[3];
    __device__ __forceinline__ PjSample(const PjLossParams& p, int n) {
        const size_t count = (size_t)p.count;
        u = p.uvs + (long long)n * p.uvs_stride;
        tg = p.target + (long long)n * p.target_stride;
        md = p.mask + (size_t)n * count;
        im = COMPOSITE ? nullptr : p.img + (long long)n * p.img_stride;
        bgi = (COMPOSITE && p.bg_image) ? p.bg_image + (long long)n * p.bg_stride : nullptr;
#pragma unroll
        for (int q = 0; q < 9; ++q) col[q] = COMPOSITE ? p.colors[(size_t)n * 9 + q] : 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) bgc[c] = (COMPOSITE && !p.bg_image) ? p.bg_color[3 * (n / p.b) + c] : 0.f;
    }
};

// partials [n, parts, 4] = {sum over foreground and channels of |target - synth|, sum over background of 1 - uvs[2], 0, 0}
template <int VEC, bool COMPOSITE>
__global__ __launch_bounds__(PJ_THREADS) void projection_loss_kernel(PjLossParams p) {
    __shared__ float wsum[PJ_THREADS / 64][2];
    const int tid = threadIdx.x, n = blockIdx.x / PJ_PARTS, part = blockIdx.x % PJ_PARTS;
    const size_t count = (size_t)p.count;
    const PjSample<VEC, COMPOSITE> s(p, n);
    float* sy = COMPOSITE ? p.synth + (size_t)n * 3 * count : nullptr;
    const int ngroups = p.count / VEC;
    const int g0 = part * p.groups_per_part, g1 = min(ngroups, g0 + p.groups_per_part);
    float v[2] = {0.f, 0.f};
    for (int g = g0 + tid; g < g1; g += PJ_THREADS) {
        const size_t o = (size_t)g * VEC;
        float u0[VEC], u1[VEC], u2[VEC];
        PjIo<VEC>::load(s.u + 2 * count + o, u2);
        if (COMPOSITE) {
            PjIo<VEC>::load(s.u + o, u0);
            PjIo<VEC>::load(s.u + count + o, u1);
        }
        const uint32_t m = PjIo<VEC>::load_mask(s.md + o);
#pragma unroll
        for (int j = 0; j < VEC; ++j) v[1] += ((m >> (8 * j)) & 1u) ? 1.f - u2[j] : 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float t[VEC], x[VEC];
            PjIo<VEC>::load(s.tg + c * count + o, t);
            if (COMPOSITE) {
                float bg[VEC];
                if (s.bgi) PjIo<VEC>::load(s.bgi + c * count + o, bg);
#pragma unroll
                for (int j = 0; j < VEC; ++j)
                    x[j] = pj_synth(pj_stroke(u0[j], u1[j], u2[j], s.col + 3 * c), 1.f - u2[j], s.bgi ? bg[j] : s.bgc[c], u2[j]);
                PjIo<VEC>::store(sy + c * count + o, x);
            } else {
                PjIo<VEC>::load(s.im + c * count + o, x);
            }
#pragma unroll
            for (int j = 0; j < VEC; ++j) v[0] += ((m >> (8 * j)) & 2u) ? fabsf(t[j] - x[j]) : 0.f;
        }
    }
    float* dst = p.partials + ((size_t)n * PJ_PARTS + part) * 4;
    pj_block_sums<2>(v, wsum, dst);
    if (tid >= 2 && tid < 4) dst[tid] = 0.f;
}

// one workgroup per exemplar: out [k,3] = {l1, bg, w_l1 l1 + w_bg bg}; an item whose count is zero is 0
__global__ __launch_bounds__(64) void projection_loss_finish_kernel(const float* __restrict__ partials, const int32_t* __restrict__ counts, int b,
                                                                    float w_l1, float w_bg, float* __restrict__ out) {
    __shared__ float item[2];
    const int tid = threadIdx.x, k = blockIdx.x;
    const float* q = partials + (size_t)k * b * PJ_PARTS * 4;
    if (tid < 2) {
        float s = 0.f;
        for (int i = 0; i < b * PJ_PARTS; ++i) s += q[(size_t)i * 4 + tid];
        const int cnt = counts[2 * k + tid];
        const float v = cnt > 0 ? s / (tid == 0 ? (float)(3ll * cnt) : (float)cnt) : 0.f;
        item[tid] = v;
        out[3 * k + tid] = v;
    }
    __syncthreads();
    if (tid == 0) out[3 * k + 2] = w_l1 * item[0] + w_bg * item[1];
}

// the gradient; with COMPOSITE partials [n, parts, 16] receive the nine sums of d_colors of the part's pixels (then seven zeros)
template <int VEC, bool COMPOSITE>
__global__ __launch_bounds__(PJ_THREADS) void projection_loss_bwd_kernel(PjLossParams p) {
    __shared__ float wsum[PJ_THREADS / 64][9];
    const int tid = threadIdx.x, n = blockIdx.x / PJ_PARTS, part = blockIdx.x % PJ_PARTS;
    const size_t count = (size_t)p.count;
    const PjSample<VEC, COMPOSITE> s(p, n);
    const int ex = n / p.b, n_fg = p.counts[2 * ex], n_bg = p.counts[2 * ex + 1];
    const float gs = p.gscale ? p.gscale[ex] : 1.f;
    const float c_l1 = n_fg > 0 ? (p.w_l1 * gs) / (float)(3ll * n_fg) : 0.f;
    const float c_bg = n_bg > 0 ? (p.w_bg * gs) / (float)n_bg : 0.f;
    const float* ds = p.d_synth ? p.d_synth + (size_t)n * 3 * count : nullptr;
    float* du = p.d_uvs + (size_t)n * 3 * count;
    float* di = COMPOSITE ? nullptr : p.d_img + (size_t)n * 3 * count;
    const int ngroups = p.count / VEC;
    const int g0 = part * p.groups_per_part, g1 = min(ngroups, g0 + p.groups_per_part);
    float v[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int g = g0 + tid; g < g1; g += PJ_THREADS) {
        const size_t o = (size_t)g * VEC;
        float u0[VEC], u1[VEC], u2[VEC], d0[VEC], d1[VEC], d2[VEC];
        PjIo<VEC>::load(s.u + 2 * count + o, u2);
        if (COMPOSITE) {
            PjIo<VEC>::load(s.u + o, u0);
            PjIo<VEC>::load(s.u + count + o, u1);
        }
        const uint32_t m = PjIo<VEC>::load_mask(s.md + o);
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            d0[j] = 0.f;
            d1[j] = 0.f;
            d2[j] = ((m >> (8 * j)) & 1u) ? -c_bg : 0.f;
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float t[VEC], x[VEC], up[VEC], bg[VEC], G[VEC];
            PjIo<VEC>::load(s.tg + c * count + o, t);
            if (ds) PjIo<VEC>::load(ds + c * count + o, up);
            if (COMPOSITE) {
                if (s.bgi) PjIo<VEC>::load(s.bgi + c * count + o, bg);
            } else {
                PjIo<VEC>::load(s.im + c * count + o, x);
            }
            const float* col = s.col + 3 * c;
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                const float a = 1.f - u2[j];
                float stroke = 0.f, bgv = 0.f;
                if (COMPOSITE) {
                    stroke = pj_stroke(u0[j], u1[j], u2[j], col);
                    bgv = s.bgi ? bg[j] : s.bgc[c];
                    x[j] = pj_synth(stroke, a, bgv, u2[j]);
                }
                const float d = x[j] - t[j];
                const float sg = ((m >> (8 * j)) & 2u) ? (d > 0.f ? c_l1 : (d < 0.f ? -c_l1 : 0.f)) : 0.f;
                G[j] = ds ? up[j] + sg : sg;
                if (COMPOSITE) {
                    d0[j] += (G[j] * col[0]) * a;
                    d1[j] += (G[j] * col[1]) * a;
                    d2[j] += G[j] * ((col[2] * a - stroke) + bgv);
                    v[3 * c + 0] += G[j] * (u0[j] * a);
                    v[3 * c + 1] += G[j] * (u1[j] * a);
                    v[3 * c + 2] += G[j] * (u2[j] * a);
                }
            }
            if (!COMPOSITE) PjIo<VEC>::store(di + c * count + o, G);
        }
        PjIo<VEC>::store(du + o, d0);
        PjIo<VEC>::store(du + count + o, d1);
        PjIo<VEC>::store(du + 2 * count + o, d2);
    }
    if (COMPOSITE) {
        float* dst = p.partials + ((size_t)n * PJ_PARTS + part) * 16;
        pj_block_sums<9>(v, wsum, dst);
        if (tid >= 9 && tid < 16) dst[tid] = 0.f;
    }
}

// d_colors [n,3,3]: the parts of a sample in their order
__global__ __launch_bounds__(256) void projection_colors_finish_kernel(const float* __restrict__ partials, int n9, float* __restrict__ d_colors) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= n9) return;
    const int n = t / 9, q = t % 9;
    float s = partials[((size_t)n * PJ_PARTS) * 16 + q];
    for (int part = 1; part < PJ_PARTS; ++part) s += partials[((size_t)n * PJ_PARTS + part) * 16 + q];
    d_colors[t] = s;
}

// what the two loss entries ask of their common arguments
static int pj_loss_args(const char* what, const float* uvs, long long uvs_stride_n, const float* colors, const float* img, long long img_stride_n,
                        const float* target, long long target_stride_n, const float* bg_image, long long bg_stride_n, const float* bg_color,
                        const uint8_t* mask, const int32_t* counts, int k, int b, int r, int composite) {
    NB_REQUIRE(uvs && target && mask && counts, "%s: null pointer", what);
    NB_REQUIRE(composite ? (colors && (bg_image || bg_color)) : img != nullptr,
               "%s: null pointer (composite needs colors and one of bg_image, bg_color; no composite needs img)", what);
    if (pj_sizes(what, k, b, r) != NB_OK) return NB_EINVAL;
    const long long count = (long long)r * r;
    NB_REQUIRE(uvs_stride_n >= 3 * count && target_stride_n >= 3 * count && (composite || img_stride_n >= 3 * count) &&
               (!(composite && bg_image) || bg_stride_n >= 3 * count), "%s: a sample stride is below 3 * r * r = %lld: the samples would alias", what, 3 * count);
    NB_REQUIRE((((uintptr_t)uvs | (uintptr_t)colors | (uintptr_t)img | (uintptr_t)target | (uintptr_t)bg_image | (uintptr_t)bg_color | (uintptr_t)counts) & 3) == 0,
               "%s: the float / int pointers must be 4-byte aligned", what);
    return NB_OK;
}

static bool pj_loss_vec(const PjLossParams& p, int composite) {
    uintptr_t a = (uintptr_t)p.uvs | (uintptr_t)p.target | (uintptr_t)p.synth | (uintptr_t)p.d_synth | (uintptr_t)p.d_uvs | (uintptr_t)p.d_img;
    long long s = p.uvs_stride | p.target_stride;
    if (composite && p.bg_image) { a |= (uintptr_t)p.bg_image; s |= p.bg_stride; }
    if (!composite) { a |= (uintptr_t)p.img; s |= p.img_stride; }
    return (p.count & 3) == 0 && (s & 3) == 0 && (a & 15) == 0 && ((uintptr_t)p.mask & 3) == 0;
}

extern "C" int nb_projection_loss_f32(const float* uvs, long long uvs_stride_n, const float* colors, const float* img, long long img_stride_n,
                                      const float* target, long long target_stride_n, const float* bg_image, long long bg_stride_n,
                                      const float* bg_color, const uint8_t* mask, const int32_t* counts, int k, int b, int r, int composite,
                                      float w_l1, float w_bg, float* synth, float* out, float* partials, void* stream) {
    if (pj_loss_args("projection_loss", uvs, uvs_stride_n, colors, img, img_stride_n, target, target_stride_n, bg_image, bg_stride_n, bg_color, mask,
                     counts, k, b, r, composite) != NB_OK) return NB_EINVAL;
    NB_REQUIRE(out && partials && (!composite || synth), "projection_loss: null pointer (out, partials; synth with composite)");
    NB_REQUIRE((((uintptr_t)synth | (uintptr_t)out | (uintptr_t)partials) & 3) == 0, "projection_loss: the float pointers must be 4-byte aligned");
    if (k == 0) return NB_OK;
    PjLossParams p{};
    p.uvs = uvs; p.uvs_stride = uvs_stride_n; p.colors = colors; p.img = img; p.img_stride = img_stride_n; p.target = target;
    p.target_stride = target_stride_n; p.bg_image = composite ? bg_image : nullptr; p.bg_stride = bg_stride_n; p.bg_color = bg_color; p.mask = mask;
    p.counts = counts; p.b = b; p.count = r * r; p.w_l1 = w_l1; p.w_bg = w_bg; p.synth = composite ? synth : nullptr; p.partials = partials;
    const bool vec = pj_loss_vec(p, composite);
    p.groups_per_part = nb_cdiv(vec ? p.count / 4 : p.count, PJ_PARTS);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(k * b * PJ_PARTS), block(PJ_THREADS);
    if (composite) {
        if (vec) hipLaunchKernelGGL((projection_loss_kernel<4, true>), grid, block, 0, st, p);
        else hipLaunchKernelGGL((projection_loss_kernel<1, true>), grid, block, 0, st, p);
    } else {
        if (vec) hipLaunchKernelGGL((projection_loss_kernel<4, false>), grid, block, 0, st, p);
        else hipLaunchKernelGGL((projection_loss_kernel<1, false>), grid, block, 0, st, p);
    }
    NB_CHECK_LAUNCH("projection_loss");
    hipLaunchKernelGGL(projection_loss_finish_kernel, dim3(k), dim3(64), 0, st, (const float*)partials, counts, b, w_l1, w_bg, out);
    NB_CHECK_LAUNCH("projection_loss_finish");
    return NB_OK;
}

extern "C" int nb_projection_loss_bwd_f32(const float* uvs, long long uvs_stride_n, const float* colors, const float* img, long long img_stride_n,
                                          const float* target, long long target_stride_n, const float* bg_image, long long bg_stride_n,
                                          const float* bg_color, const uint8_t* mask, const int32_t* counts, const float* d_synth,
                                          const float* gscale, int k, int b, int r, int composite, float w_l1, float w_bg, float* d_uvs,
                                          float* d_img, float* d_colors, float* partials, void* stream) {
    if (pj_loss_args("projection_loss_bwd", uvs, uvs_stride_n, colors, img, img_stride_n, target, target_stride_n, bg_image, bg_stride_n, bg_color,
                     mask, counts, k, b, r, composite) != NB_OK) return NB_EINVAL;
    NB_REQUIRE(d_uvs && (composite ? (d_colors && partials) : d_img != nullptr),
               "projection_loss_bwd: null pointer (d_uvs; d_colors and partials with composite, d_img without)");
    NB_REQUIRE((((uintptr_t)d_synth | (uintptr_t)gscale | (uintptr_t)d_uvs | (uintptr_t)d_img | (uintptr_t)d_colors | (uintptr_t)partials) & 3) == 0,
               "projection_loss_bwd: the float pointers must be 4-byte aligned");
    if (k == 0) return NB_OK;
    PjLossParams p{};
    p.uvs = uvs; p.uvs_stride = uvs_stride_n; p.colors = colors; p.img = img; p.img_stride = img_stride_n; p.target = target;
    p.target_stride = target_stride_n; p.bg_image = composite ? bg_image : nullptr; p.bg_stride = bg_stride_n; p.bg_color = bg_color; p.mask = mask;
    p.counts = counts; p.d_synth = d_synth; p.gscale = gscale; p.b = b; p.count = r * r; p.w_l1 = w_l1; p.w_bg = w_bg; p.d_uvs = d_uvs;
    p.d_img = composite ? nullptr : d_img; p.partials = partials;
    const bool vec = pj_loss_vec(p, composite);
    p.groups_per_part = nb_cdiv(vec ? p.count / 4 : p.count, PJ_PARTS);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(k * b * PJ_PARTS), block(PJ_THREADS);
    if (composite) {
        if (vec) hipLaunchKernelGGL((projection_loss_bwd_kernel<4, true>), grid, block, 0, st, p);
        else hipLaunchKernelGGL((projection_loss_bwd_kernel<1, true>), grid, block, 0, st, p);
        NB_CHECK_LAUNCH("projection_loss_bwd");
        hipLaunchKernelGGL(projection_colors_finish_kernel, dim3(nb_cdiv(9 * k * b, 256)), dim3(256), 0, st, (const float*)partials, 9 * k * b, d_colors);
        NB_CHECK_LAUNCH("projection_colors_finish");
    } else {
        if (vec) hipLaunchKernelGGL((projection_loss_bwd_kernel<4, false>), grid, block, 0, st, p);
        else hipLaunchKernelGGL((projection_loss_bwd_kernel<1, false>), grid, block, 0, st, p);
        NB_CHECK_LAUNCH("projection_loss_bwd");
    }
    return NB_OK;
}
