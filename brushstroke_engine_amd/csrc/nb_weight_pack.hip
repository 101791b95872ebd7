// Device weight packers (include/neube_hip.h, "device weight packers"): the packed forms the generator's layers take, built from the
// fp32 weights on the device, and the geometry encoder's conv + BatchNorm fold.  (nb_pack_conv_weight_h3_dev lives in nb_pack_h2.hip.)
#include "nb_h3_common.h"
#include "nb_gen_internal.h"

// wpk[ci][tap][co] (zero padded to ceil8(c_in) x 9 x ceil32(c_out)) = W[co][ci][tap]
__global__ __launch_bounds__(256) void gen_pack_wpk_kernel(const float* __restrict__ w, int c_out, int c_in, int co_ld, int total,
                                                           float* __restrict__ wpk) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int co = idx % co_ld, r = idx / co_ld, tap = r % 9, ci = r / 9;
    wpk[idx] = (co < c_out && ci < c_in) ? w[((size_t)co * c_in + ci) * 9 + tap] : 0.f;
}

// wsq[ci][co] = sum_k W[co][ci][k]^2 in the order of torch's reduction kernel for `w.square().sum(dim=[2, 3])` on ROCm
// (ATen/native/hip/Reduce.cuh: 9 inputs per output -> 8 lanes; lane 0 adds its two inputs 0 and 8, the lanes then combine with
// shuffle offsets 1, 2, 4), so that the demodulation coefficients of the C path equal the Python path's
__global__ __launch_bounds__(256) void gen_pack_wsq_kernel(const float* __restrict__ w, int c_out, int c_in, float* __restrict__ wsq) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= c_out * c_in) return;
    const int co = idx % c_out, ci = idx / c_out;
    const float* p = w + ((size_t)co * c_in + ci) * 9;
    float s[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) s[k] = p[k] * p[k];
    const float a = (s[0] + s[8]) + s[1], b = s[2] + s[3], c = s[4] + s[5], d = s[6] + s[7];
    wsq[idx] = (a + b) + (c + d);
}

// "f8" weights: [chunk][tap][cg][hl][ceil64(c_out)][16 bytes]; hl 0 = the 8 f16 hi halves of channel group cg, hl 1 = 16 fp8 e4m3 bytes
// over the chunk's 16 channels: w (cg 0) or (w - f16(w)) * 2^11 (cg 1), each clamped to +-448 (ops.pack_conv_weight_h3f8)
__global__ __launch_bounds__(256) void gen_pack_h3f8_kernel(const float* __restrict__ w, int c_out, int c_in, int co_ld, int nch,
                                                            uint4* __restrict__ out) {
    const int idx = blockIdx.x * 256 + threadIdx.x;             // ((chunk * 9 + tap) * 2 + cg) * co_ld + co
    if (idx >= nch * 18 * co_ld) return;
    const int co = idx % co_ld;
    int r = idx / co_ld;
    const int cg = r & 1; r >>= 1;
    const int tap = r % 9, ch = r / 9;
    auto wv = [&](int ci) -> float { return (co < c_out && ci < c_in) ? w[((size_t)co * c_in + ci) * 9 + tap] : 0.f; };
    unsigned hi[4], f8[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const _Float16 h0 = (_Float16)wv(ch * 16 + cg * 8 + 2 * j), h1 = (_Float16)wv(ch * 16 + cg * 8 + 2 * j + 1);
        hi[j] = (unsigned)__builtin_bit_cast(unsigned short, h0) | ((unsigned)__builtin_bit_cast(unsigned short, h1) << 16);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float x = wv(ch * 16 + 4 * j + k);
            v[k] = cg == 0 ? x : (x - (float)(_Float16)x) * 2048.f;
        }
        f8[j] = nb_pk2_fp8<true>(v[0], v[1]) | (nb_pk2_fp8<true>(v[2], v[3]) << 16);
    }
    const size_t base = ((((size_t)ch * 9 + tap) * 2 + cg) * 2) * co_ld;
    out[base + co] = make_uint4(hi[0], hi[1], hi[2], hi[3]);
    out[base + co_ld + co] = make_uint4(f8[0], f8[1], f8[2], f8[3]);
}

// Up=2 phase kernels folded with the FIR (ops.fold_up2_fir: Keff[2 py + px][co, ci, di + 1, dj + 1] = sum_{a, b} W[a, b] g[a - ty + 1,
// b - tx + 1], ty = py - 2 di, tx = px - 2 dj, g = flip(4 f); float64, a-major, then rounded to fp32) and packed as
// nb_pack_conv_weight_h3 per phase: out = 4 such images back to back
__global__ __launch_bounds__(256) void gen_pack_h3_up2_kernel(const float* __restrict__ w, const float* __restrict__ f, int c_out, int c_in,
                                                              int co_ld, int nch, h8* __restrict__ out) {
    const int per_phase = nch * 18 * co_ld;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= 4 * per_phase) return;
    const int ph = idx / per_phase, rem = idx % per_phase;
    const int co = rem % co_ld;
    int r = rem / co_ld;
    const int cg = r & 1; r >>= 1;
    const int tap = r % 9, ch = r / 9;
    const int py = ph >> 1, px = ph & 1, di = tap / 3 - 1, dj = tap % 3 - 1, ty = py - 2 * di, tx = px - 2 * dj;
    h8 hi, lo;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int ci = ch * 16 + cg * 8 + j;
        float v = 0.f;
        if (co < c_out && ci < c_in) {
            const float* wp = w + ((size_t)co * c_in + ci) * 9;
            double acc = 0.0;
            for (int a = 0; a < 3; ++a)
                for (int b = 0; b < 3; ++b) {
                    const int u = a - ty + 1, vv = b - tx + 1;
                    if (u >= 0 && u < 4 && vv >= 0 && vv < 4) {
                        const double g = (double)f[(3 - u) * 4 + (3 - vv)] * 4.0;
                        const double prod = (double)wp[a * 3 + b] * g;
                        acc = acc + prod;
                    }
                }
            v = (float)acc;
        }
        const _Float16 hh = (_Float16)v;
        hi[j] = hh;
        lo[j] = (_Float16)(v - (float)hh);
    }
    h8* o = out + (size_t)ph * nch * 36 * co_ld;
    const size_t base = ((((size_t)ch * 9 + tap) * 2 + cg) * 2) * co_ld;
    o[base + co] = hi;
    o[base + co_ld + co] = lo;
}

extern "C" int nb_pack_conv_weight_dev(const float* w, int c_out, int c_in, float* wpk, float* wsq, void* stream) {
    NB_REQUIRE(w && c_out > 0 && c_in > 0, "pack_conv_weight_dev: bad arguments");
    if (wpk) {
        const int total = (c_in + 7) / 8 * 8 * 9 * ((c_out + 31) / 32 * 32);
        hipLaunchKernelGGL(gen_pack_wpk_kernel, dim3(nb_cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, w, c_out, c_in,
                           (c_out + 31) / 32 * 32, total, wpk);
        NB_CHECK_LAUNCH("pack_conv_weight_dev");
    }
    if (wsq) {
        hipLaunchKernelGGL(gen_pack_wsq_kernel, dim3(nb_cdiv(c_out * c_in, 256)), dim3(256), 0, (hipStream_t)stream, w, c_out, c_in, wsq);
        NB_CHECK_LAUNCH("pack_conv_weight_dev");
    }
    return NB_OK;
}

// the f8 weight format with c_out padded to co_align (64: the generator's modconv kernels, 128: the encoder's conv kernels)
int nbgen::pack_h3f8(const float* w, int c_out, int c_in, int co_align, void* out, hipStream_t st) {
    const int nch = (c_in + 15) / 16, co_ld = (c_out + co_align - 1) / co_align * co_align;
    hipLaunchKernelGGL(gen_pack_h3f8_kernel, dim3(nb_cdiv(nch * 18 * co_ld, 256)), dim3(256), 0, st, w, c_out, c_in, co_ld, nch, (uint4*)out);
    NB_CHECK_LAUNCH("pack_conv_weight_h3f8_dev");
    return NB_OK;
}

extern "C" int nb_pack_conv_weight_h3f8_dev(const float* w, int c_out, int c_in, void* out, void* stream) {
    NB_REQUIRE(w && out && c_out > 0 && c_in > 0 && (uintptr_t)out % 16 == 0, "pack_conv_weight_h3f8_dev: bad arguments");
    return nbgen::pack_h3f8(w, c_out, c_in, 64, out, (hipStream_t)stream);
}

// The geometry encoder's conv + eval BatchNorm fold (encoder._fold_bn): s = gamma / sqrt(var + 1e-5), w' = w s, b' = (b - mean) s + beta,
// in float64 and rounded to fp32 as the numpy does.  w' [c_out][per] goes to rows of `ld` floats, zero padded (the stem's w50: per 49,
// ld 50).
__global__ __launch_bounds__(256) void enc_fold_bn_kernel(const float* __restrict__ w, const float* __restrict__ b, const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, const float* __restrict__ mean,
                                                          const float* __restrict__ var, int c_out, int per, int ld, float* __restrict__ w_out,
                                                          float* __restrict__ b_out) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= c_out * ld) return;
    const int co = idx / ld, j = idx % ld;
    const double s = (double)gamma[co] / sqrt((double)var[co] + 1e-5);
    w_out[idx] = j < per ? (float)((double)w[(size_t)co * per + j] * s) : 0.f;
    if (j == 0) b_out[co] = (float)(((double)b[co] - (double)mean[co]) * s + (double)beta[co]);
}

int nbgen::fold_bn(const float* const* p, int c_out, int per, int ld, float* w_out, float* b_out, hipStream_t st) {
    hipLaunchKernelGGL(enc_fold_bn_kernel, dim3(nb_cdiv(c_out * ld, 256)), dim3(256), 0, st, p[0], p[1], p[2], p[3], p[4], p[5], c_out, per, ld,
                       w_out, b_out);
    return hipGetLastError() == hipSuccess ? NB_OK : NB_ELAUNCH;
}

extern "C" int nb_pack_conv_weight_h3_up2_dev(const float* w, const float* resample_filter, int c_out, int c_in, void* out, void* stream) {
    NB_REQUIRE(w && resample_filter && out && c_out > 0 && c_in > 0 && (uintptr_t)out % 16 == 0, "pack_conv_weight_h3_up2_dev: bad arguments");
    const int nch = (c_in + 15) / 16, co_ld = (c_out + 63) / 64 * 64;
    hipLaunchKernelGGL(gen_pack_h3_up2_kernel, dim3(nb_cdiv(4 * nch * 18 * co_ld, 256)), dim3(256), 0, (hipStream_t)stream, w,
                       resample_filter, c_out, c_in, co_ld, nch, (h8*)out);
    NB_CHECK_LAUNCH("pack_conv_weight_h3_up2_dev");
    return NB_OK;
}
