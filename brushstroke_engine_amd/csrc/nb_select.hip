// Masked k-th largest value per image for gfx950 (painting.StyleUVSMapper.calibrate): what the reference states as
// `torch.topk(S[i][bmask[i]], k=15)[0].min()` once per calibration drawing and brush (forger/ui/mapper.py:132), for a whole batch of
// renders in one launch and without the boolean-mask gather that makes torch wait for the device.
//
// Exact radix select.  A float becomes a 32-bit key whose unsigned order is the order of torch.topk(largest=True): negative values below
// positive ones, -0 and +0 on one key, every NaN on the top key.  One 1024-thread workgroup owns one image and walks the key's four bytes
// from the top: per pass it counts, in a 256-bin LDS histogram (integer atomics: the counts do not depend on arrival order), the byte
// of every included element whose higher bytes equal the bytes chosen so far; a scan of the bins from the top finds the bin that holds
// the k-th element, and k is narrowed to a rank inside that bin.  After four passes the chosen bytes ARE the key.  The image is read
// four times (once from HBM, then from L2: an image is 64-256 KiB), in 16-byte vectors from the first 16-byte boundary of the row on;
// the up to three floats in front of it and behind the last whole vector are read one by one, so a row may start at any float.
//
// The background weight of a brush is the same to 8-16 leading bits on most of a drawing, so most lanes of a wave count into ONE bin:
// the lanes that share the first active lane's byte are counted with one atomic (ballot + popcount), the others one by one.
#include "nb_common.h"
#include <cstdint>

#define NB_SEL_THREADS 1024      // 16 waves per image: four per SIMD, so that one wave's loads are in flight under another's counting
#define NB_SEL_BINS 256

__device__ __forceinline__ uint32_t nb_sel_key(float v) {
    uint32_t u = __float_as_uint(v);
    if ((u & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;              // any NaN: above +inf (0xff800000)
    if (u == 0x80000000u) u = 0u;                                         // -0 == +0
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float nb_sel_value(uint32_t key) {
    if (key == 0xffffffffu) return __uint_as_float(0x7fc00000u);
    return __uint_as_float((key & 0x80000000u) ? (key & 0x7fffffffu) : ~key);
}

// hist[digit] += 1 for every lane with `active`; called by all lanes of the wave together
__device__ __forceinline__ void nb_sel_count(uint32_t* hist, bool active, uint32_t digit, int lane) {
    const unsigned long long act = __ballot(active);
    if (act == 0ull) return;
    const int leader = __ffsll((long long)act) - 1;
    const uint32_t d0 = (uint32_t)__shfl((int)digit, leader);
    const unsigned long long same = __ballot(active && digit == d0);
    if (lane == leader) atomicAdd(&hist[d0], (uint32_t)__popcll(same));
    if (active && digit != d0) atomicAdd(&hist[digit], 1u);
}

struct SelParams {
    const float* x;
    long long stride_n;
    const uint8_t* mask;
    int n_masks, count, k;
    float* kth;
    int32_t* n_masked;
};

__global__ __launch_bounds__(NB_SEL_THREADS) void masked_kth_largest_kernel(SelParams p) {
    __shared__ uint32_t hist[NB_SEL_BINS];
    __shared__ uint32_t wave_tot[NB_SEL_BINS / 64];
    __shared__ uint32_t sel[2];                                            // the chosen bin, and the rank inside it
    const int img = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* row = p.x + (long long)img * p.stride_n;
    const uint8_t* mrow = p.mask + (size_t)(img % p.n_masks) * (size_t)p.count;
    const int head = min(p.count, (int)(((16u - (uint32_t)((uintptr_t)row & 15u)) & 15u) >> 2));      // floats before the boundary
    const int nvec = (p.count - head) >> 2;
    const int tail0 = head + 4 * nvec, n_edge = head + (p.count - tail0);                              // n_edge <= 6
    const bool mask_words = (((uintptr_t)(mrow + head)) & 3u) == 0u;
    const float4* vrow = reinterpret_cast<const float4*>(row + head);
    uint32_t prefix = 0u, prefix_mask = 0u, k = (uint32_t)p.k;

    for (int shift = 24; shift >= 0; shift -= 8) {
        if (tid < NB_SEL_BINS) hist[tid] = 0u;
        __syncthreads();
        {   // the floats in front of the first and behind the last whole vector
            const int e = tid < head ? tid : tail0 + (tid - head);
            bool active = tid < n_edge;
            uint32_t key = 0u;
            if (active) {
                key = nb_sel_key(row[e]);
                active = mrow[e] != 0 && (key & prefix_mask) == prefix;
            }
            nb_sel_count(hist, active, (key >> shift) & 255u, lane);
        }
        for (int base = 0; base < nvec; base += NB_SEL_THREADS) {          // (the same trip count for every lane)
            const int v = base + tid;
            const bool in = v < nvec;
            float4 f = make_float4(0.f, 0.f, 0.f, 0.f);
            uint32_t m = 0u;
            if (in) {
                f = vrow[v];
                const uint8_t* mb = mrow + head + 4 * v;
                m = mask_words ? *reinterpret_cast<const uint32_t*>(mb)
                               : ((uint32_t)mb[0] | (uint32_t)mb[1] << 8 | (uint32_t)mb[2] << 16 | (uint32_t)mb[3] << 24);
            }
            const float fv[4] = {f.x, f.y, f.z, f.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t key = nb_sel_key(fv[j]);
                const bool active = ((m >> (8 * j)) & 255u) != 0u && (key & prefix_mask) == prefix;
                nb_sel_count(hist, active, (key >> shift) & 255u, lane);
            }
        }
        __syncthreads();
        // bins from the top, on the first four waves: thread t holds bin 255 - t; incl = elements in that bin and above
        const bool scans = tid < NB_SEL_BINS;                              // (whole waves)
        uint32_t c = 0u, incl = 0u;
        if (scans) {
            c = hist[NB_SEL_BINS - 1 - tid];
            incl = c;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t t = (uint32_t)__shfl_up((int)incl, o);
                if (lane >= o) incl += t;
            }
            if (lane == 63) wave_tot[wave] = incl;
        }
        __syncthreads();
        uint32_t total = 0u;
#pragma unroll
        for (int w = 0; w < NB_SEL_BINS / 64; ++w) {
            if (scans && w < wave) incl += wave_tot[w];
            total += wave_tot[w];
        }
        if (shift == 24) {
            if (tid == 0) p.n_masked[img] = (int32_t)total;
            if (total < k) {                                               // (the whole workgroup leaves together)
                if (tid == 0) p.kth[img] = __uint_as_float(0x7fc00000u);
                return;
            }
        }
        if (scans && incl - c < k && k <= incl) {                          // exactly one bin: the counts sum to >= k
            sel[0] = (uint32_t)(NB_SEL_BINS - 1 - tid);
            sel[1] = k - (incl - c);
        }
        __syncthreads();
        prefix |= sel[0] << shift;
        prefix_mask |= 255u << shift;
        k = sel[1];
    }
    if (tid == 0) p.kth[img] = nb_sel_value(prefix);
}

extern "C" int nb_masked_kth_largest_f32(const float* x, long long stride_n, const uint8_t* mask, int n_masks, int count, int k, int n,
                                         float* kth, int32_t* n_masked, void* stream) {
    NB_REQUIRE(x && mask && kth && n_masked, "masked_kth_largest: null pointer");
    NB_REQUIRE(k >= 1, "masked_kth_largest: k = %d, must be at least 1", k);
    NB_REQUIRE(count >= 1 && n_masks >= 1 && n >= 0, "masked_kth_largest: bad sizes (count %d, n_masks %d, n %d)", count, n_masks, n);
    NB_REQUIRE(stride_n >= (long long)count, "masked_kth_largest: stride_n %lld below count %d: the images would alias", stride_n, count);
    NB_REQUIRE((((uintptr_t)x | (uintptr_t)kth | (uintptr_t)n_masked) & 3) == 0, "masked_kth_largest: x, kth and n_masked must be 4-byte aligned");
    if (n == 0) return NB_OK;
    SelParams p{x, stride_n, mask, n_masks, count, k, kth, n_masked};
    hipLaunchKernelGGL(masked_kth_largest_kernel, dim3(n), dim3(NB_SEL_THREADS), 0, (hipStream_t)stream, p);
    NB_CHECK_LAUNCH("masked_kth_largest");
    return NB_OK;
}
