// Clarity optimisation of brushes for gfx950 (clarity.ClarityOptimizer): everything of one step of the reference's
// run_one_clarity_opt (scripts/opt_clarity_main.py:93-167) that is not the generator, for K brushes at once.
//
// The state of K brushes is one arena [K, P] of floats, a row = W+ (nw floats) followed by the noise planes (NbClarityPlanes: side
// and offset of each, validated on the host before anything is launched and handed to the kernels by value).
//
//   nb_clarity_loss_f32      the default loss without its perceptual item, 0.5*iou_inv(uvs)+0.5*iou(u)+50*l1(fake_orig)
//                            (forger/train/losses.py:453-474, 501-530, 649-666): NB_CLARITY_LOSS_PARTS workgroups share a sample and
//                            leave five partial sums, a second launch adds them in their order and forms the per-brush items.
//   nb_clarity_loss_bwd_f32  the gradient with respect to uvs and the image from those sums, one thread per pixel.
//   nb_noise_reg_f32         the multi-scale noise regulariser (opt_clarity_main.py:127-137), value and gradient.  Pass 1: a workgroup
//                            takes a tile of a plane with a halo of one cell of the COARSEST level to its left and above (read with
//                            wrap-around), builds the 2x2-mean pyramid of that region in LDS, writes its own cells of the levels >= 1
//                            to scratch and leaves the tile's sums of n * roll_x n and n * roll_y n per level.  Pass 2: a workgroup adds
//                            the sums of its plane in their order and evaluates, per level-0 pixel,
//                                sum_l 4^-l [2 a_l / N_l (left + right) + 2 b_l / N_l (up + down)]   at (y >> l, x >> l), wrapping,
//                            reading level 0 from the arena and the other levels from scratch.
//   nb_clarity_step_f32      Adam (torch.optim.Adam's arithmetic, bias-corrected) over the whole arena with the sums of n and n^2 per
//                            chunk of a plane, then n = (n - mean) * rsqrt(mean((n - mean)^2)) per plane (opt_clarity_main.py:163-167).
//
// fp32 throughout, no float atomics: every sum is lanes by halving, waves one after the other, workgroups one after the other, so
// the same input gives the same bits and row k of a K-row call equals the one-row call on that row.
#include "nb_common.h"
#include <cstdint>
#include <cmath>

#define CL_THREADS 256
#define CL_PARTS NB_CLARITY_LOSS_PARTS
#define CL_CHUNK NB_CLARITY_CHUNK
#define CL_MAXP NB_CLARITY_MAX_PLANES
#define CL_MAX_RES 256                                                     // (tile + halo)^2 and its pyramid must fit in 64 KiB of LDS
#define CL_TILE 64
#define CL_LDS_FLOATS 12288                                                // 96^2 * (1 + 1/4 + 1/16 + ...) < 96^2 * 4 / 3
#define CL_MAX_LEVELS 6                                                    // 256, 128, 64, 32, 16, 8

struct ClLayout {
    int n_planes, nw;
    int res[CL_MAXP], off[CL_MAXP];
    int tile0[CL_MAXP + 1];                                                // pass-1 tiles of the regulariser: plane i owns tile0[i] .. tile0[i+1]
    int pyr0[CL_MAXP + 1];                                                 // levels >= 1 of plane i in a row's pyramid scratch
    int chunk0[CL_MAXP + 2];                                               // chunks of CL_CHUNK floats: segment 0 = W+, segment i + 1 = plane i
};

static inline int cl_levels(int res) { int n = 1; while ((res >> (n - 1)) > 8) ++n; return n; }
static inline int cl_tile(int res) { return res < CL_TILE ? res : CL_TILE; }

// Validates the plane table against a row of p floats whose first nw are W+, and lays out tiles, pyramid scratch and chunks.
static int cl_layout(const NbClarityPlanes* planes, int nw, long long p, const char* what, ClLayout& L) {
    NB_REQUIRE(planes, "%s: null pointer (planes)", what);
    NB_REQUIRE(planes->n >= 0 && planes->n <= CL_MAXP, "%s: bad plane count %d (0..%d)", what, planes->n, CL_MAXP);
    NB_REQUIRE(nw >= 0 && p >= nw && p <= (1ll << 30), "%s: bad row sizes (nw %d, p %lld)", what, nw, p);
    L.n_planes = planes->n;
    L.nw = nw;
    long long end = nw;
    L.tile0[0] = 0; L.pyr0[0] = 0; L.chunk0[0] = 0; L.chunk0[1] = nb_cdiv(nw, CL_CHUNK);
    for (int i = 0; i < planes->n; ++i) {
        const int r = planes->res[i], o = planes->off[i];
        NB_REQUIRE(r >= 4 && r <= CL_MAX_RES && (r & (r - 1)) == 0, "%s: plane %d has side %d: a power of two in 4..%d is supported", what, i, r, CL_MAX_RES);
        NB_REQUIRE(o >= end && (long long)o + (long long)r * r <= p, "%s: plane %d (side %d, offset %d) overlaps what precedes it or leaves the row of %lld floats",
                   what, i, r, o, p);
        end = (long long)o + (long long)r * r;
        L.res[i] = r; L.off[i] = o;
        const int t = r / cl_tile(r);
        L.tile0[i + 1] = L.tile0[i] + t * t;
        int pyr = 0;
        for (int l = 1; l < cl_levels(r); ++l) pyr += (r >> l) * (r >> l);
        L.pyr0[i + 1] = L.pyr0[i] + pyr;
        L.chunk0[i + 2] = L.chunk0[i + 1] + nb_cdiv(r * r, CL_CHUNK);
    }
    for (int i = planes->n; i < CL_MAXP; ++i) { L.res[i] = 0; L.off[i] = 0; L.tile0[i + 1] = L.tile0[i]; L.pyr0[i + 1] = L.pyr0[i]; L.chunk0[i + 2] = L.chunk0[i + 1]; }
    return NB_OK;
}
static inline long long cl_reg_floats(const ClLayout& L) { return 16ll * L.tile0[L.n_planes] + L.pyr0[L.n_planes]; }
static inline long long cl_step_floats(const ClLayout& L) { return 2ll * L.chunk0[L.n_planes + 1]; }

extern "C" long long nb_clarity_scratch_floats(const NbClarityPlanes* planes, int nw, long long p, int k) {
    ClLayout L;
    if (cl_layout(planes, nw, p, "clarity_scratch_floats", L) != NB_OK) return -1;
    if (k < 0 || k > 65535) { nb_set_error("clarity_scratch_floats: k %d outside 0..65535", k); return -1; }
    const long long a = cl_reg_floats(L), b = cl_step_floats(L);
    return (long long)k * (a > b ? a : b);
}

// the last i with prefix[i] <= x (prefix[0] == 0, n entries)
__device__ __forceinline__ int cl_find(const int* prefix, int n, int x) {
    int i = 0;
    while (i + 1 < n && prefix[i + 1] <= x) ++i;
    return i;
}

__device__ __forceinline__ float cl_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_down(v, o);
    return v;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// loss
// ---------------------------------------------------------------------------------------------------------------------------------
struct ClLossParams {
    const float* uvs; long long uvs_stride;
    const float* img; long long img_stride;
    const float* target; long long target_stride;
    const float* geom;
    int b, count, per_part;
};

__global__ __launch_bounds__(CL_THREADS) void clarity_loss_kernel(ClLossParams p, float* __restrict__ partials) {
    __shared__ float wsum[CL_THREADS / 64][5];
    const int tid = threadIdx.x, n = blockIdx.x / CL_PARTS, part = blockIdx.x % CL_PARTS;
    const size_t count = (size_t)p.count;
    const float* u = p.uvs + (long long)n * p.uvs_stride;
    const float* s = u + 2 * count;
    const float* im = p.img + (long long)n * p.img_stride;
    const float* tg = p.target + (long long)n * p.target_stride;
    const float* g = p.geom + (size_t)(n % p.b) * count;
    const int e0 = part * p.per_part, e1 = min(p.count, e0 + p.per_part);
    float v[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    for (int e = e0 + tid; e < e1; e += CL_THREADS) {
        const float gg = g[e], t = 1.f - gg, ss = s[e], uu = u[e];
        v[0] += ss * gg;
        v[1] += ss + gg;
        v[2] += uu * t;
        v[3] += uu + t;
        v[4] += fabsf(im[e] - tg[e]);
        v[4] += fabsf(im[count + e] - tg[count + e]);
        v[4] += fabsf(im[2 * count + e] - tg[2 * count + e]);
    }
#pragma unroll
    for (int q = 0; q < 5; ++q) v[q] = cl_wave_sum(v[q]);
    if ((tid & 63) == 0) {
#pragma unroll
        for (int q = 0; q < 5; ++q) wsum[tid >> 6][q] = v[q];
    }
    __syncthreads();
    if (tid < 8) {
        float r = 0.f;
        if (tid < 5) {
            r = wsum[0][tid];
            for (int w = 1; w < CL_THREADS / 64; ++w) r += wsum[w][tid];
        }
        partials[((size_t)n * CL_PARTS + part) * 8 + tid] = r;
    }
}

// one workgroup per brush: sums[n, 8] = {I_s, U_s, I_u, U_u, sum |img - target|, 0, 0, 0}, out[k, 4] = the three items and their weighted sum
__global__ __launch_bounds__(CL_THREADS) void clarity_loss_finish_kernel(const float* __restrict__ partials, int b, int count, float w_inv, float w_iou,
                                                                         float w_l1, float* sums, float* __restrict__ out) {
    const int tid = threadIdx.x, k = blockIdx.x;
    for (int idx = tid; idx < b * 8; idx += CL_THREADS) {
        const size_t n = (size_t)k * b + idx / 8;
        const int q = idx % 8;
        float s = partials[n * CL_PARTS * 8 + q];
        for (int part = 1; part < CL_PARTS; ++part) s += partials[(n * CL_PARTS + part) * 8 + q];
        sums[n * 8 + q] = s;
    }
    __syncthreads();
    if (tid == 0) {
        const float eps = 1e-8f;
        float acc_inv = 0.f, acc_iou = 0.f, acc_l1 = 0.f;
        for (int i = 0; i < b; ++i) {
            float* s = sums + ((size_t)k * b + i) * 8;
            const float us = (s[1] - s[0]) + eps, uu = (s[3] - s[2]) + eps;
            acc_inv += s[0] / us;
            acc_iou += s[2] / uu;
            acc_l1 += s[4];
            s[1] = us;
            s[3] = uu;
        }
        const float o0 = 1.f - acc_inv / (float)b, o1 = 1.f - acc_iou / (float)b, o2 = acc_l1 / (float)(3ll * b * count);
        out[4 * k + 0] = o0;
        out[4 * k + 1] = o1;
        out[4 * k + 2] = o2;
        out[4 * k + 3] = (w_inv * o0 + w_iou * o1) + w_l1 * o2;
    }
}

static int cl_loss_sizes(const char* what, int k, int b, int r) {
    NB_REQUIRE(k >= 0 && b >= 1 && r >= 1 && r <= 4096 && (long long)k * b <= 65535,
               "%s: bad sizes (k %d, b %d, r %d; k >= 0, b >= 1, r in 1..4096, k * b <= 65535)", what, k, b, r);
    return NB_OK;
}

extern "C" int nb_clarity_loss_f32(const float* uvs, long long uvs_stride_n, const float* img, long long img_stride_n, const float* target,
                                   long long target_stride_n, const float* geom, int k, int b, int r, float w_iou_inv, float w_iou, float w_l1,
                                   float* out, float* sums, float* partials, void* stream) {
    NB_REQUIRE(uvs && img && target && geom && out && sums && partials, "clarity_loss: null pointer");
    if (cl_loss_sizes("clarity_loss", k, b, r) != NB_OK) return NB_EINVAL;
    const long long count = (long long)r * r;
    NB_REQUIRE(uvs_stride_n >= 3 * count && img_stride_n >= 3 * count && target_stride_n >= 3 * count,
               "clarity_loss: a sample stride is below 3 * r * r = %lld: the samples would alias", 3 * count);
    NB_REQUIRE((((uintptr_t)uvs | (uintptr_t)img | (uintptr_t)target | (uintptr_t)geom | (uintptr_t)out | (uintptr_t)sums | (uintptr_t)partials) & 3) == 0,
               "clarity_loss: the float pointers must be 4-byte aligned");
    if (k == 0) return NB_OK;
    hipStream_t st = (hipStream_t)stream;
    ClLossParams p{uvs, uvs_stride_n, img, img_stride_n, target, target_stride_n, geom, b, (int)count, nb_cdiv((int)count, CL_PARTS)};
    hipLaunchKernelGGL(clarity_loss_kernel, dim3(k * b * CL_PARTS), dim3(CL_THREADS), 0, st, p, partials);
    NB_CHECK_LAUNCH("clarity_loss");
    hipLaunchKernelGGL(clarity_loss_finish_kernel, dim3(k), dim3(CL_THREADS), 0, st, (const float*)partials, b, (int)count, w_iou_inv, w_iou, w_l1, sums, out);
    NB_CHECK_LAUNCH("clarity_loss_finish");
    return NB_OK;
}

struct ClBwdParams {
    const float* img; long long img_stride;
    const float* target; long long target_stride;
    const float* geom; const float* sums; const float* gscale;
    int b, count;
    float w_inv, w_iou, w_l1;
    float* d_uvs; float* d_img;
};

__global__ __launch_bounds__(CL_THREADS) void clarity_loss_bwd_kernel(ClBwdParams p) {
    const int e = blockIdx.x * CL_THREADS + threadIdx.x, n = blockIdx.y;
    if (e >= p.count) return;
    const size_t count = (size_t)p.count;
    const float gs = p.gscale ? p.gscale[n / p.b] : 1.f;
    const float* s = p.sums + (size_t)n * 8;
    const float i_s = s[0], u_s = s[1], i_u = s[2], u_u = s[3];
    const float g = p.geom[(size_t)(n % p.b) * count + e], t = 1.f - g;
    const float c_inv = -(p.w_inv * gs) / (float)p.b, c_iou = -(p.w_iou * gs) / (float)p.b;
    const float c_l1 = (p.w_l1 * gs) / (float)(3ll * p.b * p.count);
    float* du = p.d_uvs + (size_t)n * 3 * count;
    du[e] = c_iou * ((t * u_u - i_u * (1.f - t)) / (u_u * u_u));
    du[count + e] = 0.f;
    du[2 * count + e] = c_inv * ((g * u_s - i_s * (1.f - g)) / (u_s * u_s));
    const float* im = p.img + (long long)n * p.img_stride;
    const float* tg = p.target + (long long)n * p.target_stride;
    float* di = p.d_img + (size_t)n * 3 * count;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float d = im[c * count + e] - tg[c * count + e];
        di[c * count + e] = d > 0.f ? c_l1 : (d < 0.f ? -c_l1 : 0.f);
    }
}

extern "C" int nb_clarity_loss_bwd_f32(const float* img, long long img_stride_n, const float* target, long long target_stride_n, const float* geom,
                                       const float* sums, const float* gscale, int k, int b, int r, float w_iou_inv, float w_iou, float w_l1,
                                       float* d_uvs, float* d_img, void* stream) {
    NB_REQUIRE(img && target && geom && sums && d_uvs && d_img, "clarity_loss_bwd: null pointer");
    if (cl_loss_sizes("clarity_loss_bwd", k, b, r) != NB_OK) return NB_EINVAL;
    const long long count = (long long)r * r;
    NB_REQUIRE(img_stride_n >= 3 * count && target_stride_n >= 3 * count,
               "clarity_loss_bwd: a sample stride is below 3 * r * r = %lld: the samples would alias", 3 * count);
    NB_REQUIRE((((uintptr_t)img | (uintptr_t)target | (uintptr_t)geom | (uintptr_t)sums | (uintptr_t)gscale | (uintptr_t)d_uvs | (uintptr_t)d_img) & 3) == 0,
               "clarity_loss_bwd: the float pointers must be 4-byte aligned");
    if (k == 0) return NB_OK;
    ClBwdParams p{img, img_stride_n, target, target_stride_n, geom, sums, gscale, b, (int)count, w_iou_inv, w_iou, w_l1, d_uvs, d_img};
    hipLaunchKernelGGL(clarity_loss_bwd_kernel, dim3(nb_cdiv((int)count, CL_THREADS), k * b), dim3(CL_THREADS), 0, (hipStream_t)stream, p);
    NB_CHECK_LAUNCH("clarity_loss_bwd");
    return NB_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// noise regulariser
// ---------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int cl_dev_levels(int res) { int n = 1; while ((res >> (n - 1)) > 8) ++n; return n; }

// pass 1.  scratch row k: [tiles_total][16] tile sums (2 l + 0: sum n roll_x n, 2 l + 1: sum n roll_y n), then the pyramid levels >= 1
__global__ __launch_bounds__(CL_THREADS) void noise_reg_sums_kernel(ClLayout L, const float* __restrict__ arena, long long row_stride,
                                                                    float* __restrict__ scratch, long long scratch_row) {
    __shared__ float lv[CL_LDS_FLOATS];
    __shared__ float wsum[CL_MAX_LEVELS][CL_THREADS / 64][2];
    const int tid = threadIdx.x, k = blockIdx.y, tile = blockIdx.x;
    const int i = cl_find(L.tile0, L.n_planes + 1, tile);
    const int R = L.res[i], ts = R < CL_TILE ? R : CL_TILE, tiles_x = R / ts, lt = tile - L.tile0[i];
    const int ty0 = (lt / tiles_x) * ts, tx0 = (lt % tiles_x) * ts;
    const int nlev = cl_dev_levels(R), H = 1 << (nlev - 1), E = ts + H;
    const float* plane = arena + (long long)k * row_stride + L.off[i];
    float* tile_sums = scratch + (long long)k * scratch_row + (size_t)tile * 16;
    float* pyr = scratch + (long long)k * scratch_row + (size_t)L.tile0[L.n_planes] * 16 + L.pyr0[i];
    for (int e = tid; e < E * E; e += CL_THREADS) {                        // level 0 of tile + halo, wrapping around the plane
        const int ly = e / E, lx = e % E, y = (ty0 - H + ly) & (R - 1), x = (tx0 - H + lx) & (R - 1);
        lv[e] = plane[y * R + x];
    }
    __syncthreads();
    int src = 0, lvl_pyr = 0;
    for (int l = 0; l < nlev; ++l) {
        const int El = E >> l, Hl = H >> l, Tl = ts >> l, Rl = R >> l;
        if (l > 0) {                                                       // level l from level l - 1, its own cells out to scratch
            const int Ep = E >> (l - 1), dst = src + Ep * Ep;
            for (int e = tid; e < El * El; e += CL_THREADS) {
                const int cy = e / El, cx = e % El;
                const float* q = lv + src + (2 * cy) * Ep + 2 * cx;
                const float m = (((q[0] + q[1]) + q[Ep]) + q[Ep + 1]) * 0.25f;
                lv[dst + e] = m;
                if (cy >= Hl && cx >= Hl) pyr[lvl_pyr + ((ty0 >> l) + cy - Hl) * Rl + (tx0 >> l) + cx - Hl] = m;
            }
            src = dst;
            __syncthreads();
        }
        float a = 0.f, bsum = 0.f;
        for (int e = tid; e < Tl * Tl; e += CL_THREADS) {
            const int cy = Hl + e / Tl, cx = Hl + e % Tl;
            const float c = lv[src + cy * El + cx];
            a += c * lv[src + cy * El + cx - 1];
            bsum += c * lv[src + (cy - 1) * El + cx];
        }
        a = cl_wave_sum(a);
        bsum = cl_wave_sum(bsum);
        if ((tid & 63) == 0) { wsum[l][tid >> 6][0] = a; wsum[l][tid >> 6][1] = bsum; }
        if (l > 0) lvl_pyr += Rl * Rl;
    }
    __syncthreads();
    if (tid < 16) {
        float s = 0.f;
        const int l = tid >> 1, q = tid & 1;
        if (l < nlev) {
            s = wsum[l][0][q];
            for (int w = 1; w < CL_THREADS / 64; ++w) s += wsum[l][w][q];
        }
        tile_sums[tid] = s;
    }
}

// the sums of plane i's tiles in their order: a_l (q = 0) or b_l (q = 1) as a mean over the level's N_l cells
__device__ __forceinline__ float cl_level_mean(const ClLayout& L, const float* tiles, int i, int l, int q) {
    float s = 0.f;
    for (int t = L.tile0[i]; t < L.tile0[i + 1]; ++t) s += tiles[(size_t)t * 16 + 2 * l + q];
    const int Rl = L.res[i] >> l;
    return s / (float)(Rl * Rl);
}

// pass 2: the gradient of a chunk of a plane, added times `weight` into grad; the workgroup of a row's first chunk also leaves reg[k]
__global__ __launch_bounds__(CL_THREADS) void noise_reg_grad_kernel(ClLayout L, const float* __restrict__ arena, long long row_stride,
                                                                    const float* __restrict__ scratch, long long scratch_row, float weight,
                                                                    float* __restrict__ grad, long long grad_stride, float* __restrict__ reg) {
    __shared__ float coef[CL_MAX_LEVELS][2];
    __shared__ float plane_reg[CL_MAXP];
    const int tid = threadIdx.x, k = blockIdx.y, chunk = blockIdx.x;
    const float* tiles = scratch + (long long)k * scratch_row;
    if (chunk == 0) {
        if (tid < L.n_planes) {
            float s = 0.f;
            for (int l = 0; l < cl_dev_levels(L.res[tid]); ++l) {
                const float a = cl_level_mean(L, tiles, tid, l, 0), b = cl_level_mean(L, tiles, tid, l, 1);
                s += a * a;
                s += b * b;
            }
            plane_reg[tid] = s;
        }
        __syncthreads();
        if (tid == 0) {
            float s = 0.f;
            for (int i = 0; i < L.n_planes; ++i) s += plane_reg[i];
            reg[k] = s;
        }
    }
    const int seg = cl_find(L.chunk0, L.n_planes + 2, chunk);
    if (seg == 0 || grad == nullptr) return;                              // W+ takes no part
    const int i = seg - 1, R = L.res[i], nlev = cl_dev_levels(R), sh = 31 - __clz(R);
    if (tid < 2 * nlev) {
        const int l = tid >> 1, Rl = R >> l;
        coef[l][tid & 1] = (2.f * cl_level_mean(L, tiles, i, l, tid & 1)) / (float)(Rl * Rl) * (1.f / (float)(1 << (2 * l)));
    }
    __syncthreads();
    const float* plane = arena + (long long)k * row_stride + L.off[i];
    const float* pyr = tiles + (size_t)L.tile0[L.n_planes] * 16 + L.pyr0[i];
    float* gp = grad + (long long)k * grad_stride + L.off[i];
    const int e0 = (chunk - L.chunk0[seg]) * CL_CHUNK;
    for (int j = 0; j < CL_CHUNK / CL_THREADS; ++j) {
        const int e = e0 + j * CL_THREADS + tid;
        if (e >= R * R) break;
        const int y = e >> sh, x = e & (R - 1);
        float g = 0.f;
        const float* src = plane;
        for (int l = 0; l < nlev; ++l) {
            const int Rl = R >> l, m = Rl - 1, cy = y >> l, cx = x >> l;
            const float lr = src[cy * Rl + ((cx - 1) & m)] + src[cy * Rl + ((cx + 1) & m)];
            const float ud = src[((cy - 1) & m) * Rl + cx] + src[((cy + 1) & m) * Rl + cx];
            g += coef[l][0] * lr + coef[l][1] * ud;
            src = l == 0 ? pyr : src + Rl * Rl;
        }
        gp[e] += weight * g;
    }
}

extern "C" int nb_noise_reg_f32(const float* arena, long long row_stride, long long p, int nw, const NbClarityPlanes* planes, int k, float weight,
                                float* grad, long long grad_stride, float* reg, float* scratch, long long scratch_floats, void* stream) {
    NB_REQUIRE(arena && reg && scratch, "noise_reg: null pointer");
    ClLayout L;
    if (cl_layout(planes, nw, p, "noise_reg", L) != NB_OK) return NB_EINVAL;
    NB_REQUIRE(k >= 0 && k <= 65535, "noise_reg: k %d outside 0..65535", k);
    NB_REQUIRE(row_stride >= p && (grad == nullptr || grad_stride >= p), "noise_reg: a row stride is below p = %lld: the rows would alias", p);
    NB_REQUIRE((((uintptr_t)arena | (uintptr_t)grad | (uintptr_t)reg | (uintptr_t)scratch) & 3) == 0, "noise_reg: the float pointers must be 4-byte aligned");
    const long long per_row = cl_reg_floats(L);
    NB_REQUIRE(scratch_floats >= (long long)k * per_row, "noise_reg: scratch of %lld floats is too small: %lld needed (nb_clarity_scratch_floats)",
               scratch_floats, (long long)k * per_row);
    if (k == 0) return NB_OK;
    hipStream_t st = (hipStream_t)stream;
    if (L.n_planes == 0) {                                                 // nothing to regularise: the value is zero, the gradient untouched
        if (hipMemsetAsync(reg, 0, sizeof(float) * (size_t)k, st) != hipSuccess) {
            (void)hipGetLastError();
            nb_set_error("noise_reg: clearing the values failed");
            return NB_ELAUNCH;
        }
        return NB_OK;
    }
    hipLaunchKernelGGL(noise_reg_sums_kernel, dim3(L.tile0[L.n_planes], k), dim3(CL_THREADS), 0, st, L, arena, row_stride, scratch, per_row);
    NB_CHECK_LAUNCH("noise_reg_sums");
    hipLaunchKernelGGL(noise_reg_grad_kernel, dim3(L.chunk0[L.n_planes + 1], k), dim3(CL_THREADS), 0, st, L, arena, row_stride, (const float*)scratch,
                       per_row, weight, grad, grad_stride, reg);
    NB_CHECK_LAUNCH("noise_reg_grad");
    return NB_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// step
// ---------------------------------------------------------------------------------------------------------------------------------
struct ClAdam { float one_minus_b1, b2, one_minus_b2, step_size, bc2_sqrt, eps; };

__global__ __launch_bounds__(CL_THREADS) void clarity_step_update_kernel(ClLayout L, ClAdam A, float* __restrict__ arena, const float* __restrict__ grad,
                                                                         float* __restrict__ m_, float* __restrict__ v_, long long row_stride,
                                                                         float* __restrict__ partials) {
    __shared__ float wsum[CL_THREADS / 64][2];
    const int tid = threadIdx.x, k = blockIdx.y, chunk = blockIdx.x;
    const int seg = cl_find(L.chunk0, L.n_planes + 2, chunk);
    const int len = seg == 0 ? L.nw : L.res[seg - 1] * L.res[seg - 1];
    const long long base = (long long)k * row_stride + (seg == 0 ? 0 : L.off[seg - 1]);
    const int e0 = (chunk - L.chunk0[seg]) * CL_CHUNK;
    float s1 = 0.f, s2 = 0.f;
    for (int j = 0; j < CL_CHUNK / CL_THREADS; ++j) {
        const int e = e0 + j * CL_THREADS + tid;
        if (e >= len) break;
        const float g = grad[base + e];
        float m = m_[base + e], v = v_[base + e], x = arena[base + e];
        m = m + (g - m) * A.one_minus_b1;                                  // exp_avg.lerp_(grad, 1 - beta1)
        v = v * A.b2 + (A.one_minus_b2 * g) * g;                           // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
        const float denom = sqrtf(v) / A.bc2_sqrt + A.eps;
        x = x - A.step_size * (m / denom);                                 // param.addcdiv_(exp_avg, denom, value=-step_size)
        m_[base + e] = m;
        v_[base + e] = v;
        arena[base + e] = x;
        s1 += x;
        s2 += x * x;
    }
    s1 = cl_wave_sum(s1);
    s2 = cl_wave_sum(s2);
    if ((tid & 63) == 0) { wsum[tid >> 6][0] = s1; wsum[tid >> 6][1] = s2; }
    __syncthreads();
    if (tid < 2) {
        float s = wsum[0][tid];
        for (int w = 1; w < CL_THREADS / 64; ++w) s += wsum[w][tid];
        partials[((size_t)k * L.chunk0[L.n_planes + 1] + chunk) * 2 + tid] = s;
    }
}

__global__ __launch_bounds__(CL_THREADS) void clarity_step_norm_kernel(ClLayout L, float* __restrict__ arena, long long row_stride,
                                                                       const float* __restrict__ partials) {
    __shared__ float tot[2];
    const int tid = threadIdx.x, k = blockIdx.y, chunk = blockIdx.x;
    const int seg = cl_find(L.chunk0, L.n_planes + 2, chunk);
    if (seg == 0) return;                                                  // W+ is not normalised
    const int R = L.res[seg - 1], len = R * R;
    if (tid < 2) {
        const float* q = partials + (size_t)k * L.chunk0[L.n_planes + 1] * 2;
        float s = 0.f;
        for (int c = L.chunk0[seg]; c < L.chunk0[seg + 1]; ++c) s += q[2 * c + tid];
        tot[tid] = s;
    }
    __syncthreads();
    const float mean = tot[0] / (float)len;
    const float scale = 1.f / sqrtf(tot[1] / (float)len - mean * mean);    // mean((n - mean)^2)
    float* x = arena + (long long)k * row_stride + L.off[seg - 1];
    const int e0 = (chunk - L.chunk0[seg]) * CL_CHUNK;
    for (int j = 0; j < CL_CHUNK / CL_THREADS; ++j) {
        const int e = e0 + j * CL_THREADS + tid;
        if (e >= len) break;
        x[e] = (x[e] - mean) * scale;
    }
}

extern "C" int nb_clarity_step_f32(float* arena, const float* grad, float* m, float* v, long long row_stride, long long p, int nw,
                                   const NbClarityPlanes* planes, int k, float lr, int t, float* scratch, long long scratch_floats, void* stream) {
    NB_REQUIRE(arena && grad && m && v && scratch, "clarity_step: null pointer");
    ClLayout L;
    if (cl_layout(planes, nw, p, "clarity_step", L) != NB_OK) return NB_EINVAL;
    NB_REQUIRE(k >= 0 && k <= 65535 && t >= 1, "clarity_step: bad counts (k %d outside 0..65535 or step t %d below 1)", k, t);
    NB_REQUIRE(row_stride >= p, "clarity_step: row stride %lld below p = %lld: the rows would alias", row_stride, p);
    NB_REQUIRE((((uintptr_t)arena | (uintptr_t)grad | (uintptr_t)m | (uintptr_t)v | (uintptr_t)scratch) & 3) == 0,
               "clarity_step: the float pointers must be 4-byte aligned");
    const long long need = (long long)k * cl_step_floats(L);
    NB_REQUIRE(scratch_floats >= need, "clarity_step: scratch of %lld floats is too small: %lld needed (nb_clarity_scratch_floats)", scratch_floats, need);
    if (k == 0 || L.chunk0[L.n_planes + 1] == 0) return NB_OK;
    const double b1 = 0.9, b2 = 0.999;
    ClAdam A{(float)(1.0 - b1), (float)b2, (float)(1.0 - b2), (float)((double)lr / (1.0 - std::pow(b1, (double)t))),
             (float)std::sqrt(1.0 - std::pow(b2, (double)t)), 1e-8f};
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(L.chunk0[L.n_planes + 1], k);
    hipLaunchKernelGGL(clarity_step_update_kernel, grid, dim3(CL_THREADS), 0, st, L, A, arena, grad, m, v, row_stride, scratch);
    NB_CHECK_LAUNCH("clarity_step_update");
    if (L.n_planes > 0) {
        hipLaunchKernelGGL(clarity_step_norm_kernel, grid, dim3(CL_THREADS), 0, st, L, arena, row_stride, (const float*)scratch);
        NB_CHECK_LAUNCH("clarity_step_norm");
    }
    return NB_OK;
}
