// Operand packers of the split-f16 convolutions: fp32 NCHW activations -> the H2 / "f8" / "f6" formats, fp32 weights -> the
// hi/lo f16 weight format (formats: nb_modconv_up1_h3.hip, nb_h3_common.h).
#include "nb_h3_common.h"

// ------------------------------------------------------------------------------------------------
// fp32 NCHW -> H2 packing (optionally x two concatenated inputs, x per-(n,c) scale = the consumer's styles)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pack_h2_kernel(const float* __restrict__ x1, int c1, const float* __restrict__ x2, int c2,
                                                      const float* __restrict__ scale, _Float16* __restrict__ out, int c8, int hw) {
    const int n = blockIdx.z, cg = blockIdx.y;
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= hw) return;
    const int c_in = c1 + c2;
    h8 hi, lo;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int ch = cg * 8 + j;
        float v = 0.f;
        if (ch < c_in) {
            v = ch < c1 ? x1[((size_t)n * c1 + ch) * hw + pix] : x2[((size_t)n * c2 + (ch - c1)) * hw + pix];
            if (scale) v *= scale[(size_t)n * c_in + ch];
        }
        const _Float16 hh = (_Float16)v;
        hi[j] = hh;
        lo[j] = (_Float16)(v - (float)hh);
    }
    h8* o = reinterpret_cast<h8*>(out) + ((size_t)(n * c8 + cg) * 2) * hw + pix;
    o[0] = hi;
    o[hw] = lo;
}

extern "C" int nb_pack_h2_f32(const float* x1, int c1, const float* x2, int c2, const float* scale, void* out_h2, int n,
                              int hw, void* stream) {
    NB_REQUIRE(x1 && out_h2 && c1 > 0 && c2 >= 0 && (c2 == 0 || x2) && n > 0 && n <= 65535 && hw > 0, "pack_h2: bad arguments");
    const int c8 = (c1 + c2 + 7) / 8;
    dim3 grid((hw + 255) / 256, c8, n);
    hipLaunchKernelGGL(pack_h2_kernel, grid, dim3(256), 0, (hipStream_t)stream, x1, c1, x2, c2, scale, (_Float16*)out_h2, c8, hw);
    NB_CHECK_LAUNCH("pack_h2");
    return NB_OK;
}

// fp32 NCHW (x1 ++ x2) * scale -> the "f8" activation format (see modconv3x3_up1_h3_kernel): per 16-channel chunk the
// f16 high halves of both channel groups, fp8(xl * 2^9) and fp8(x / 4)
__global__ __launch_bounds__(256) void pack_h2f8_kernel(const float* __restrict__ x1, int c1, const float* __restrict__ x2, int c2,
                                                        const float* __restrict__ scale, _Float16* __restrict__ out, int c8, int hw) {
    const int n = blockIdx.z, chunk = blockIdx.y;
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= hw) return;
    const int c_in = c1 + c2;
    float v[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int ch = chunk * 16 + j;
        float t = 0.f;
        if (ch < c_in) {
            t = ch < c1 ? x1[((size_t)n * c1 + ch) * hw + pix] : x2[((size_t)n * c2 + (ch - c1)) * hw + pix];
            if (scale) t *= scale[(size_t)n * c_in + ch];
        }
        v[j] = t;
    }
    h8 hi0, hi1;
    float xl[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const _Float16 hh = (_Float16)v[j];
        if (j < 8) hi0[j & 7] = hh; else hi1[j & 7] = hh;
        xl[j] = (v[j] - (float)hh) * 512.f;
    }
    i32x4 l8, h8v;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        l8[q] = (int)nb_pk4_fp8(xl[4 * q], xl[4 * q + 1], xl[4 * q + 2], xl[4 * q + 3]);
        h8v[q] = (int)nb_pk4_fp8(v[4 * q] * 0.25f, v[4 * q + 1] * 0.25f, v[4 * q + 2] * 0.25f, v[4 * q + 3] * 0.25f);
    }
    h8* o = reinterpret_cast<h8*>(out) + ((size_t)(n * c8 + 2 * chunk) * 2) * hw + pix;
    o[0] = hi0;
    o[hw] = __builtin_bit_cast(h8, l8);
    o[2 * (size_t)hw] = hi1;
    o[3 * (size_t)hw] = __builtin_bit_cast(h8, h8v);
}

extern "C" int nb_pack_h2f8_f32(const float* x1, int c1, const float* x2, int c2, const float* scale, void* out, int n, int hw,
                                void* stream) {
    NB_REQUIRE(x1 && out && c1 > 0 && c2 >= 0 && (c2 == 0 || x2) && n > 0 && n <= 65535 && hw > 0, "pack_h2f8: bad arguments");
    NB_REQUIRE((c1 + c2) % 16 == 0, "pack_h2f8: the f8 operand format needs a multiple of 16 channels (got %d)", c1 + c2);
    const int c8 = (c1 + c2) / 8;
    dim3 grid((hw + 255) / 256, c8 / 2, n);
    hipLaunchKernelGGL(pack_h2f8_kernel, grid, dim3(256), 0, (hipStream_t)stream, x1, c1, x2, c2, scale, (_Float16*)out, c8, hw);
    NB_CHECK_LAUNCH("pack_h2f8");
    return NB_OK;
}

// fp32 NCHW (x1 ++ x2) * scale -> the "f6" activation format (nb_h3_common.h): per 16-channel chunk the f16 high halves of both channel
// groups and, in the two lo slots, 32 e2m3 fields (xl 2^11 / S, x / S interleaved) + the chunk's scale byte.  With cg0 / c8_total:
// into channel groups cg0.. of a tensor with c8_total groups (the geometry features behind a producer that wrote its own groups).
__global__ __launch_bounds__(256) void pack_h2f6_kernel(const float* __restrict__ x1, int c1, const float* __restrict__ x2, int c2,
                                                        const float* __restrict__ scale, int scale_stride, _Float16* __restrict__ out,
                                                        int c8_total, int cg0, int hw) {
    const int n = blockIdx.z, chunk = blockIdx.y;
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= hw) return;
    const int c_in = c1 + c2;
    float v[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int ch = chunk * 16 + j;
        float t = 0.f;
        if (ch < c_in) {
            t = ch < c1 ? x1[((size_t)n * c1 + ch) * hw + pix] : x2[((size_t)n * c2 + (ch - c1)) * hw + pix];
            if (scale) t *= scale[(size_t)n * scale_stride + ch];
        }
        v[j] = t;
    }
    h8 hi0, hi1;
    i32x4 l0, l1;
    nb_f6_encode16(v, hi0, hi1, l0, l1);
    h8* o = reinterpret_cast<h8*>(out) + ((size_t)(n * c8_total + cg0 + 2 * chunk) * 2) * hw + pix;
    o[0] = hi0;
    o[hw] = __builtin_bit_cast(h8, l0);
    o[2 * (size_t)hw] = hi1;
    o[3 * (size_t)hw] = __builtin_bit_cast(h8, l1);
}

extern "C" int nb_pack_h2f6_f32(const float* x1, int c1, const float* x2, int c2, const float* scale, void* out, int n, int hw,
                                void* stream) {
    NB_REQUIRE(x1 && out && c1 > 0 && c2 >= 0 && (c2 == 0 || x2) && n > 0 && n <= 65535 && hw > 0, "pack_h2f6: bad arguments");
    NB_REQUIRE((c1 + c2) % 16 == 0, "pack_h2f6: the f6 operand format needs a multiple of 16 channels (got %d)", c1 + c2);
    const int c8 = (c1 + c2) / 8;
    dim3 grid((hw + 255) / 256, c8 / 2, n);
    hipLaunchKernelGGL(pack_h2f6_kernel, grid, dim3(256), 0, (hipStream_t)stream, x1, c1, x2, c2, scale, c1 + c2, (_Float16*)out, c8, 0, hw);
    NB_CHECK_LAUNCH("pack_h2f6");
    return NB_OK;
}

extern "C" int nb_pack_h2f6_part_f32(const float* x, int c, const float* scale, int scale_stride, void* out, int c8_total,
                                     int cg0, int n, int hw, void* stream) {
    NB_REQUIRE(x && out && c > 0 && c % 16 == 0 && cg0 % 2 == 0 && n > 0 && n <= 65535 && hw > 0 && cg0 >= 0 && cg0 + c / 8 <= c8_total,
               "pack_h2f6_part: bad arguments (whole 16-channel chunks only)");
    dim3 grid((hw + 255) / 256, c / 16, n);
    hipLaunchKernelGGL(pack_h2f6_kernel, grid, dim3(256), 0, (hipStream_t)stream, x, c, (const float*)nullptr, 0, scale, scale_stride, (_Float16*)out,
                       c8_total, cg0, hw);
    NB_CHECK_LAUNCH("pack_h2f6_part");
    return NB_OK;
}

// Pack c channels of an fp32 NCHW tensor into channel groups cg0.. of an H2 tensor with c8_total groups (the geometry
// features that the consumer concatenates behind a producer that wrote its own groups directly)
__global__ __launch_bounds__(256) void pack_h2_part_kernel(const float* __restrict__ x, int c, const float* __restrict__ scale,
                                                           int scale_stride, _Float16* __restrict__ out, int c8_total, int cg0, int hw) {
    const int n = blockIdx.z, cgl = blockIdx.y;
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= hw) return;
    h8 hi, lo;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int ch = cgl * 8 + j;
        float v = 0.f;
        if (ch < c) {
            v = x[((size_t)n * c + ch) * hw + pix];
            if (scale) v *= scale[(size_t)n * scale_stride + ch];
        }
        const _Float16 hh = (_Float16)v;
        hi[j] = hh;
        lo[j] = (_Float16)(v - (float)hh);
    }
    h8* o = reinterpret_cast<h8*>(out) + ((size_t)(n * c8_total + cg0 + cgl) * 2) * hw + pix;
    o[0] = hi;
    o[hw] = lo;
}

__global__ __launch_bounds__(256) void pack_h2f8_part_kernel(const float* __restrict__ x, int c, const float* __restrict__ scale,
                                                             int scale_stride, _Float16* __restrict__ out, int c8_total, int cg0, int hw) {
    const int n = blockIdx.z, chunk = blockIdx.y;
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= hw) return;
    float v[16], xl[16];
    h8 hi0, hi1;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int ch = chunk * 16 + j;
        float t = 0.f;
        if (ch < c) {
            t = x[((size_t)n * c + ch) * hw + pix];
            if (scale) t *= scale[(size_t)n * scale_stride + ch];
        }
        const _Float16 hh = (_Float16)t;
        if (j < 8) hi0[j & 7] = hh; else hi1[j & 7] = hh;
        v[j] = t; xl[j] = (t - (float)hh) * 512.f;
    }
    i32x4 l8, h8v;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        l8[q] = (int)nb_pk4_fp8(xl[4 * q], xl[4 * q + 1], xl[4 * q + 2], xl[4 * q + 3]);
        h8v[q] = (int)nb_pk4_fp8(v[4 * q] * 0.25f, v[4 * q + 1] * 0.25f, v[4 * q + 2] * 0.25f, v[4 * q + 3] * 0.25f);
    }
    h8* o = reinterpret_cast<h8*>(out) + ((size_t)(n * c8_total + cg0 + 2 * chunk) * 2) * hw + pix;
    o[0] = hi0;
    o[hw] = __builtin_bit_cast(h8, l8);
    o[2 * (size_t)hw] = hi1;
    o[3 * (size_t)hw] = __builtin_bit_cast(h8, h8v);
}

extern "C" int nb_pack_h2f8_part_f32(const float* x, int c, const float* scale, int scale_stride, void* out, int c8_total,
                                     int cg0, int n, int hw, void* stream) {
    NB_REQUIRE(x && out && c > 0 && c % 16 == 0 && cg0 % 2 == 0 && n > 0 && n <= 65535 && hw > 0 && cg0 >= 0 && cg0 + c / 8 <= c8_total,
               "pack_h2f8_part: bad arguments (whole 16-channel chunks only)");
    dim3 grid((hw + 255) / 256, c / 16, n);
    hipLaunchKernelGGL(pack_h2f8_part_kernel, grid, dim3(256), 0, (hipStream_t)stream, x, c, scale, scale_stride, (_Float16*)out, c8_total, cg0, hw);
    NB_CHECK_LAUNCH("pack_h2f8_part");
    return NB_OK;
}

extern "C" int nb_pack_h2_part_f32(const float* x, int c, const float* scale, int scale_stride, void* out_h2, int c8_total,
                                   int cg0, int n, int hw, void* stream) {
    NB_REQUIRE(x && out_h2 && c > 0 && n > 0 && n <= 65535 && hw > 0 && cg0 >= 0 && cg0 + (c + 7) / 8 <= c8_total, "pack_h2_part: bad arguments");
    dim3 grid((hw + 255) / 256, (c + 7) / 8, n);
    hipLaunchKernelGGL(pack_h2_part_kernel, grid, dim3(256), 0, (hipStream_t)stream, x, c, scale, scale_stride, (_Float16*)out_h2, c8_total, cg0, hw);
    NB_CHECK_LAUNCH("pack_h2_part");
    return NB_OK;
}

// Device-side weight packing (same layout as the host helper below): one thread per (chunk, tap, cg, co) writes the hi and lo
// slots of its 8 channels (zero padding included)
// tf != 0: w is the weight of the convolution whose INPUT gradient is being computed, [c_in][c_out][3][3] in this call's terms; the
// packed weight is its transpose with the taps reversed (the transposed convolution's kernel) -- no flipped copy in between.
__global__ __launch_bounds__(256) void pack_conv_weight_h3_kernel(const float* __restrict__ w, int c_out, int c_in, int co_ld, int nch,
                                                                  h8* __restrict__ out, int tf) {
    const int idx = blockIdx.x * 256 + threadIdx.x;             // ((chunk * 9 + tap) * 2 + cg) * co_ld + co
    if (idx >= nch * 18 * co_ld) return;
    const int co = idx % co_ld;
    int r = idx / co_ld;
    const int cg = r & 1; r >>= 1;
    const int tap = r % 9, ch = r / 9;
    h8 hi, lo;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int ci = ch * 16 + cg * 8 + j;
        const float v = (co < c_out && ci < c_in) ? (tf ? w[((size_t)ci * c_out + co) * 9 + 8 - tap] : w[((size_t)co * c_in + ci) * 9 + tap]) : 0.f;
        const _Float16 hh = (_Float16)v;
        hi[j] = hh;
        lo[j] = (_Float16)(v - (float)hh);
    }
    const size_t base = ((((size_t)ch * 9 + tap) * 2 + cg) * 2) * co_ld;
    out[base + co] = hi;
    out[base + co_ld + co] = lo;
}

extern "C" int nb_pack_conv_weight_h3_dev(const float* w, int c_out, int c_in, int co_align, int transpose_flip, void* out, void* stream) {
    NB_REQUIRE(w && out && c_out > 0 && c_in > 0 && (uintptr_t)out % 16 == 0 && (co_align == 64 || co_align == 128), "pack_conv_weight_h3_dev: bad arguments");
    const int nch = (c_in + 15) / 16, co_ld = (c_out + co_align - 1) / co_align * co_align;
    const int total = nch * 18 * co_ld;
    hipLaunchKernelGGL(pack_conv_weight_h3_kernel, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, w, c_out, c_in, co_ld, nch,
                       (h8*)out, transpose_flip);
    NB_CHECK_LAUNCH("pack_conv_weight_h3_dev");
    return NB_OK;
}

// Host-side weight packing: W[c_out][c_in][3][3] fp32 -> hi/lo f16 [ceil16(c_in)/16][3][3][2][2][ceil64(c_out)][8]
extern "C" int nb_pack_conv_weight_h3(const float* w, int c_out, int c_in, void* out) {
    NB_REQUIRE(w && out && c_out > 0 && c_in > 0, "pack_conv_weight_h3: bad arguments");
    const int nch = (c_in + 15) / 16, co_ld = (c_out + 63) / 64 * 64;
    _Float16* o = (_Float16*)out;
    const size_t total = (size_t)nch * 9 * 4 * co_ld * 8;
    for (size_t i = 0; i < total; ++i) o[i] = (_Float16)0.f;
    for (int co = 0; co < c_out; ++co)
        for (int ci = 0; ci < c_in; ++ci)
            for (int t = 0; t < 9; ++t) {
                const float v = w[((size_t)co * c_in + ci) * 9 + t];
                const _Float16 hi = (_Float16)v;
                const _Float16 lo = (_Float16)(v - (float)hi);
                const int ch = ci / 16, cg = (ci % 16) / 8, j = ci % 8;
                const size_t base = ((((size_t)ch * 9 + t) * 2 + cg) * 2) * co_ld;
                o[(base + co) * 8 + j] = hi;
                o[(base + co_ld + co) * 8 + j] = lo;
            }
    return NB_OK;
}
