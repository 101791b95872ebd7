// The whole generator behind one C handle (include/neube_hip.h, "the whole generator"): device weight packers, the parameter and
// layer tables of a GeneratorConfig, and the host orchestration of one forward pass -- the launches and per-batch kernel choices of
// SynthesisNetwork._run_layers (networks.py) on one stream, without torch.
//
// The per-batch kernel decisions of a pass live in one place, the planner (nb_synthesis_plan): SynthesisNetwork and the walk below
// both follow its plan.  The orchestration is a single walk (gen_walk) used two ways: to size the workspaces at creation (every
// batch up to n_max, whole passes and every stage) and to enqueue a forward pass -- whole, or one stage of the painting engine's
// split (NbGeneratorStage: a head that stops after a block, a tail that resumes behind it).  It differs from SynthesisNetwork only in
// that the early geometry pack runs in-line on the one stream instead of on a side stream (same kernel, same inputs: same bits).
#include "nb_h3_common.h"
#include <cmath>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

// ------------------------------------------------------------------------------------------------
// device weight packers
// ------------------------------------------------------------------------------------------------

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
static int pack_h3f8(const float* w, int c_out, int c_in, int co_align, void* out, hipStream_t st) {
    const int nch = (c_in + 15) / 16, co_ld = (c_out + co_align - 1) / co_align * co_align;
    hipLaunchKernelGGL(gen_pack_h3f8_kernel, dim3(nb_cdiv(nch * 18 * co_ld, 256)), dim3(256), 0, st, w, c_out, c_in, co_ld, nch, (uint4*)out);
    NB_CHECK_LAUNCH("pack_conv_weight_h3f8_dev");
    return NB_OK;
}

extern "C" int nb_pack_conv_weight_h3f8_dev(const float* w, int c_out, int c_in, void* out, void* stream) {
    NB_REQUIRE(w && out && c_out > 0 && c_in > 0 && (uintptr_t)out % 16 == 0, "pack_conv_weight_h3f8_dev: bad arguments");
    return pack_h3f8(w, c_out, c_in, 64, out, (hipStream_t)stream);
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

extern "C" int nb_pack_conv_weight_h3_up2_dev(const float* w, const float* resample_filter, int c_out, int c_in, void* out, void* stream) {
    NB_REQUIRE(w && resample_filter && out && c_out > 0 && c_in > 0 && (uintptr_t)out % 16 == 0, "pack_conv_weight_h3_up2_dev: bad arguments");
    const int nch = (c_in + 15) / 16, co_ld = (c_out + 63) / 64 * 64;
    hipLaunchKernelGGL(gen_pack_h3_up2_kernel, dim3(nb_cdiv(4 * nch * 18 * co_ld, 256)), dim3(256), 0, (hipStream_t)stream, w,
                       resample_filter, c_out, c_in, co_ld, nch, (h8*)out);
    NB_CHECK_LAUNCH("pack_conv_weight_h3_up2_dev");
    return NB_OK;
}

// ------------------------------------------------------------------------------------------------
// small helpers of the generator object
// ------------------------------------------------------------------------------------------------

// dst[i] = src[i * stride] (noise_lin = noise_grid[0, :, 0, 0])
__global__ __launch_bounds__(256) void gen_gather_kernel(const float* __restrict__ src, int stride, int count, float* __restrict__ dst) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < count) dst[i] = src[(size_t)i * stride];
}

// dst[x * r + y] = src[y * r + x] (noise_const_t)
__global__ __launch_bounds__(256) void gen_transpose_kernel(const float* __restrict__ src, int r, float* __restrict__ dst) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < r * r) dst[i] = src[(i % r) * r + i / r];
}

// dst[k * count + i] = src[i] for k < reps (the learned constant repeated over the batch)
__global__ __launch_bounds__(256) void gen_repeat_kernel(const float* __restrict__ src, int count, int reps, float* __restrict__ dst) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < count * reps) dst[i] = src[i % count];
}

// Truncation (networks.py:283-289): ws[:, :cutoff] = lerp(w_avg, ws, psi), in the form of torch's lerp (the small-weight branch
// below 0.5); the summation in torch may differ in the last bit
__global__ __launch_bounds__(256) void gen_truncate_kernel(float* __restrict__ ws, const float* __restrict__ w_avg, float psi, int n,
                                                           int num_ws, int w_dim, int cutoff) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int per = cutoff * w_dim;
    if (i >= n * per) return;
    const int s = i / per, r = i % per;
    float* p = ws + (size_t)s * num_ws * w_dim + r;
    const float a = w_avg[r % w_dim], b = *p;
    *p = fabsf(psi) < 0.5f ? a + psi * (b - a) : b - (b - a) * (1.f - psi);
}

// ------------------------------------------------------------------------------------------------
// configuration: parameter and layer tables (config.GeneratorConfig, weights.random_state_dict)
// ------------------------------------------------------------------------------------------------
namespace {

struct GenLayer {
    std::string name;
    int block_res, up, in_ch, out_ch, geom_ch, w_index;
    int in_res() const { return block_res / up; }
};

struct GenParam {
    std::string name;
    int ndim;
    int64_t shape[4];
    int64_t numel() const { int64_t v = 1; for (int k = 0; k < ndim; ++k) v *= shape[k]; return v; }
};

struct GenCfg {
    NbGeneratorConfig c;
    int R = 0;
    std::vector<int> blocks, geom_res, geom_ch;
    std::vector<GenLayer> layers;
    std::vector<GenParam> params;
    int num_ws = 0;
    int channels(int res) const { return std::min(c.channel_base / res, c.channel_max); }
    int geom_index(int res) const {
        for (size_t k = 0; k < geom_res.size(); ++k)
            if (geom_res[k] == res) return (int)k;
        return -1;
    }
};

std::string fmt(const char* f, int a) {
    char b[96];
    snprintf(b, sizeof(b), f, a);
    return b;
}

void add_param(GenCfg& g, const std::string& name, std::initializer_list<int64_t> shape) {
    GenParam p;
    p.name = name;
    p.ndim = (int)shape.size();
    int k = 0;
    for (int64_t v : shape) p.shape[k++] = v;
    for (; k < 4; ++k) p.shape[k] = 0;
    g.params.push_back(p);
}

// validates and expands a configuration; NB_EINVAL (with nb_last_error) on anything GeneratorConfig would reject or this path
// does not take
int resolve_cfg(const NbGeneratorConfig* c, GenCfg& g) {
    NB_REQUIRE(c, "generator: null config");
    const int R = c->img_resolution;
    NB_REQUIRE(c->c_dim == 0, "generator: c_dim must be 0 (conditioning labels are not part of this path)");
    NB_REQUIRE(c->z_dim >= 1 && c->z_dim <= 512 && c->w_dim >= 1 && c->w_dim <= 512, "generator: z_dim and w_dim must be in [1, 512]");
    NB_REQUIRE(R >= 4 && R <= 4096 && (R & (R - 1)) == 0, "generator: img_resolution must be a power of two >= 4");
    NB_REQUIRE(c->mapping_layers >= 1 && c->mapping_layers <= 64, "generator: mapping_layers must be in [1, 64]");
    NB_REQUIRE(c->mapping_lr_multiplier > 0.f, "generator: mapping_lr_multiplier must be positive");
    NB_REQUIRE(c->channel_max >= 1 && c->channel_base / R >= 1, "generator: channel_base / img_resolution and channel_max must be >= 1");
    NB_REQUIRE(c->num_geom >= 0 && c->num_geom <= 4, "generator: num_geom must be in [0, 4]");
    g.c = *c;
    g.R = R;
    for (int r = 4; r <= R; r *= 2) g.blocks.push_back(r);
    bool all_zero = true;
    for (int k = 0; k < c->num_geom; ++k) all_zero = all_zero && c->geom_resolutions[k] == 0;
    for (int k = 0; k < c->num_geom; ++k) {
        NB_REQUIRE(c->geom_channels[k] >= 1 && c->geom_channels[k] <= 4096, "generator: geom_channels[%d] must be in [1, 4096]", k);
        g.geom_ch.push_back(c->geom_channels[k]);
        if (all_zero) {
            NB_REQUIRE(c->num_geom == 2, "generator: the default geometry resolutions (R/8, R/4) need num_geom == 2");
            g.geom_res.push_back(k == 0 ? R / 8 : R / 4);
        } else {
            g.geom_res.push_back(c->geom_resolutions[k]);
        }
        const int gr = g.geom_res.back();
        NB_REQUIRE(gr >= 4 && gr < R && (gr & (gr - 1)) == 0, "generator: geometry resolution %d must be a power of two in [4, R/2]", gr);
        for (int j = 0; j < k; ++j) NB_REQUIRE(g.geom_res[j] != gr, "generator: geometry resolution %d given twice", gr);
    }
    int w = 0;
    for (int res : g.blocks) {
        const int oc = g.channels(res);
        if (res > 4) {
            const int gi = g.geom_index(res / 2);
            const int gc = gi < 0 ? 0 : g.geom_ch[gi];
            g.layers.push_back({fmt("synthesis.b%d.conv0", res), res, 2, g.channels(res / 2) + gc, oc, gc, w++});
        }
        g.layers.push_back({fmt("synthesis.b%d.conv1", res), res, 1, oc, oc, 0, w++});
    }
    g.num_ws = (int)g.layers.size() + 1;
    // the state dict, in the order of weights.random_state_dict
    for (int i = 0; i < c->mapping_layers; ++i) {
        add_param(g, fmt("mapping.fc%d.weight", i), {c->w_dim, i == 0 ? c->z_dim : c->w_dim});
        add_param(g, fmt("mapping.fc%d.bias", i), {c->w_dim});
    }
    add_param(g, "mapping.w_avg", {c->w_dim});
    add_param(g, "synthesis.b4.const", {g.channels(4), 4, 4});
    for (int res : g.blocks) add_param(g, fmt("synthesis.b%d.resample_filter", res), {4, 4});
    for (const GenLayer& l : g.layers) {
        add_param(g, l.name + ".weight", {l.out_ch, l.in_ch, 3, 3});
        add_param(g, l.name + ".noise_strength", {});
        add_param(g, l.name + ".bias", {l.out_ch});
        add_param(g, l.name + ".noise_grid", {1, l.block_res, l.block_res, 2});
        add_param(g, l.name + ".resample_filter", {4, 4});
        add_param(g, l.name + ".noise_const", {l.block_res, l.block_res});
        add_param(g, l.name + ".affine.weight", {l.in_ch, c->w_dim});
        add_param(g, l.name + ".affine.bias", {l.in_ch});
    }
    const std::string t = fmt("synthesis.b%d.torgb", R);
    const int cl = g.channels(R);
    add_param(g, t + ".weight", {3, cl, 1, 1});
    add_param(g, t + ".bias", {3});
    add_param(g, t + ".color_bias", {9});
    add_param(g, t + ".affine.weight", {cl + 9, c->w_dim});
    add_param(g, t + ".affine.bias", {cl + 9});
    return NB_OK;
}

int copy_name(const std::string& s, char* buf, int len) {
    if (!buf) return NB_OK;
    NB_REQUIRE(len > (int)s.size(), "generator: name buffer too short (%d bytes for \"%s\")", len, s.c_str());
    memcpy(buf, s.c_str(), s.size() + 1);
    return NB_OK;
}

// ------------------------------------------------------------------------------------------------
// the per-batch layer plan (nb_synthesis_plan): every kernel decision of SynthesisNetwork's pass and of gen_walk
// ------------------------------------------------------------------------------------------------

int plan_pass(const GenCfg& g, const NbPlanOptions& o, int n, NbPassPlan* p) {
    NB_REQUIRE(p, "synthesis_plan: null output");
    NB_REQUIRE(n >= 1 && n <= 65535, "synthesis_plan: batch %d outside [1, 65535]", n);
    NB_REQUIRE(o.conv_mode >= NB_CONV_F32 && o.conv_mode <= NB_CONV_F16, "synthesis_plan: unknown conv_mode %d", o.conv_mode);
    NB_REQUIRE(o.noise_positions >= NB_PLAN_POS_NONE && o.noise_positions <= NB_PLAN_POS_NORM, "synthesis_plan: bad noise_positions %d",
               o.noise_positions);
    const int nL = (int)g.layers.size(), ng = (int)g.geom_res.size(), mode = o.conv_mode;
    NB_REQUIRE(nL <= NB_PLAN_MAX_LAYERS && ng <= 4, "synthesis_plan: %d layers, at most %d", nL, NB_PLAN_MAX_LAYERS);
    memset(p, 0, sizeof(*p));
    p->num_layers = nL;
    p->num_geom = ng;
    const bool split = mode != NB_CONV_F32;                                   // large layers on the split-f16 kernel family
    const bool f8 = mode == NB_CONV_F8 || mode == NB_CONV_F6 || mode == NB_CONV_F16;      // ... f8 operands where c_in allows
    const bool has_clamp = g.c.conv_clamp >= 0.f;
    const bool clamp_ok = has_clamp && g.c.conv_clamp <= 1024.f;             // activations bounded inside the f16 range
    auto bit = [](int mask, int res) { return (mask >> __builtin_ctz(res)) & 1; };

    // the large split-f16 kernels: up=1 needs rows of 32 pixels; up=2 inputs of 32k pixel rows, or 16 / 8 (8 x 16 / 8 x 8 quad
    // tiles: few workgroups per sample, so only from a batch); both enough output pixels to fill the chip with large workgroups
    auto large = [&](const GenLayer& s) {
        if (!split || !clamp_ok || n < o.h3_min_batch) return false;
        const bool px = (long long)n * s.block_res * s.block_res >= o.h3_min_pixels;
        if (s.up == 1) return s.block_res >= 32 && s.block_res % 32 == 0 && px;
        const int ir = s.in_res();
        const bool w8 = ir == 8 && n >= o.h3_up2_w8_min_batch;
        return ((ir >= 32 && ir % 32 == 0) || (ir == 16 && n >= o.h3_up2_w16_min_batch) || w8) && (w8 || px);
    };
    // operand format of a large layer's input: 1 = f8 (whole 16-channel chunks only), 0 = H2; 2 = f6 in conv_mode f6 for the up=2
    // launches on the software-pipelined up2v kernel (their producers, an up=1 kernel or the geometry pack, write it; the up=2
    // epilogue does not, so the up=1 layers behind an up=2 layer stay on f8)
    int rc = NB_OK;
    auto operand_fmt = [&](const GenLayer& s) {
        if (!f8 || s.in_ch % 16) return 0;
        if (mode == NB_CONV_F6 && s.up == 2 && s.in_res() % 32 == 0) {
            char v[64];
            const int r = nb_modconv3x3_up2_h3_variant(2, s.in_ch, s.out_ch, n, s.in_res(), s.in_res(), v, sizeof(v));
            if (r) rc = r;
            if (!r && strcmp(v, "modconv3x3_up2v_kernel") == 0) return 2;
        }
        return 1;
    };

    // ---- the pass ----
    const bool positional = o.noise_positions != NB_PLAN_POS_NONE;
    // (16-byte friendly shapes; the squared styles of a layer fit in the fast kernel's LDS array, the ToRGB's c + 9 included)
    bool styles_fast = o.styles_fast && g.c.w_dim % 16 == 0 && g.channels(g.R) + 9 <= NB_MAX_AFF;
    for (const GenLayer& s : g.layers) styles_fast = styles_fast && s.out_ch % 4 == 0 && s.in_ch <= NB_MAX_AFF;
    p->styles_fast = styles_fast;
    // small batches: styles and per-sample noise in one launch (a launch costs more than either computes)
    p->styles_noise = styles_fast && positional && !o.noise_overrides && n <= 8;
    // the in-kernel noise tiles normalise integer positions per tile; from batch 9 one launch normalises them for the batch
    p->positions_once = o.positions_once && o.noise_positions == NB_PLAN_POS_INT && n > 8;
    // from this layer on every layer runs on the large kernels, which compute their shifted noise in their prologue (not with
    // per-call noise overrides: nobody has transposed those; a brush noise set keeps its transposes and is no override)
    p->inkernel_from = -1;
    if (o.noise_in_kernel && positional && !o.noise_overrides) {
        int k = nL;
        while (k > 0 && large(g.layers[k - 1])) --k;
        p->inkernel_from = k < nL ? k : -1;
    }

    // ---- the layers ----
    for (int i = 0; i < nL; ++i) {
        const GenLayer& s = g.layers[i];
        const GenLayer* nxt = i + 1 < nL ? &g.layers[i + 1] : nullptr;
        NbLayerPlan& L = p->layers[i];
        const int res = s.block_res, ir = s.in_res();
        const bool is_last = res == g.R;
        L.noise_in_kernel = p->inkernel_from >= 0 && i >= p->inkernel_from;
        if (split && has_clamp) {
            L.packs = NB_PACK_H3;
            if (f8 && s.in_ch % 16 == 0) L.packs |= NB_PACK_F8 | (mode == NB_CONV_F6 && s.up == 2 ? NB_PACK_F6 : 0);
            if (s.up == 2 && ir <= 32 && s.in_ch % 16 == 0) L.packs |= NB_PACK_H3_UP2;
        }
        if (large(s)) {
            L.kind = NB_KERNEL_LARGE_H3;
            L.in_fmt = operand_fmt(s);
            L.kernel_fmt = mode == NB_CONV_F16 && L.in_fmt == 1 ? 3 : L.in_fmt;
            // the operand hand-off: both ends large and nothing reads the fp32 activations in between; whole 8-channel groups
            // (16 for f8 operands, the geometry channels behind them included); f6 operands only from an f8 / f6 up=1 loop
            const bool tapped = s.up == 1 && (is_last || bit(o.tap_mask | o.blend_mask, res));
            const int out_fmt = nxt && large(*nxt) ? operand_fmt(*nxt) : 0;
            const int gi = s.up == 1 ? g.geom_index(res) : -1;
            const int geo_after = gi < 0 ? 0 : g.geom_ch[gi];
            L.handoff = o.h2_handoff && nxt && large(*nxt) && !tapped && s.out_ch % 8 == 0
                && (out_fmt == 0 || (s.out_ch % 16 == 0 && geo_after % 16 == 0)) && (out_fmt != 2 || (L.in_fmt != 0 && s.up == 1));
            L.out_fmt = L.handoff ? out_fmt : 0;
            L.fused_torgb = o.fuse_torgb && is_last && s.up == 1 && s.out_ch <= 128 && !bit(o.blend_mask, res);
            if (s.up == 1)
                snprintf(L.kernel, sizeof(L.kernel), "modconv3x3_up1_h3_kernel<%d>", s.out_ch > 64 ? 2 : 1);
            else if (const int r = nb_modconv3x3_up2_h3_variant(L.in_fmt, s.in_ch, s.out_ch, n, ir, ir, L.kernel, sizeof(L.kernel)))
                return r;
            continue;
        }
        // the small-image split-f16 kernels: <= 64x64 conv1 layers, conv0 layers with inputs <= 32x32 (FIR folded into four
        // per-phase kernels); whole 16-channel chunks, the geometry channels included
        const bool small_ok = o.small_h3 && split && clamp_ok && s.in_ch % 16 == 0 && s.in_ch <= 512;
        if (small_ok && ((s.up == 1 && res <= 64) || (s.up == 2 && (L.packs & NB_PACK_H3_UP2) && s.geom_ch % 16 == 0))) {
            L.kind = NB_KERNEL_SMALL_H3;
            snprintf(L.kernel, sizeof(L.kernel), "modconv3x3_up1_small_h3_kernel");
        } else if (const int r = nb_modconv3x3_variant(n, ir, ir, s.out_ch, s.up, L.kernel, sizeof(L.kernel))) {
            return r;
        }
    }

    // ---- the geometry features: packed into their consumer's operands (not for a block the pass resumes after or whose
    // fp32 output is tapped or blended) ----
    for (int gi = 0; gi < ng; ++gi) {
        NbGeomPlan& G = p->geom[gi];
        const int gres = g.geom_res[gi], gch = g.geom_ch[gi];
        G.consumer = -1;
        for (int i = 0; i + 1 < nL; ++i)
            if (g.layers[i].block_res == gres && g.layers[i].up == 1) G.consumer = i + 1;
        if (G.consumer < 0 || (o.resume_res && gres <= o.resume_res) || bit(o.tap_mask | o.blend_mask, gres)) continue;
        const GenLayer &sp = g.layers[G.consumer - 1], &sc = g.layers[G.consumer];
        if (!(large(sp) && large(sc))) continue;
        const int ofmt = operand_fmt(sc);
        G.early_pack = o.early_geom_pack && o.h2_handoff && sp.out_ch % 8 == 0 && (ofmt == 0 || (sp.out_ch % 16 == 0 && gch % 16 == 0));
        // (feature 0 also feeds the encoder's own decoder: it stays fp32; the encoder's epilogue writes H2 / f8 operands only)
        G.encoder_handoff = o.h2_handoff && gi == 1 && ofmt != 2 && sp.out_ch % 16 == 0 && gch % 16 == 0;
        G.fmt = G.early_pack || G.encoder_handoff ? ofmt : 0;
    }
    return rc;
}

}  // namespace

extern "C" int nb_plan_options_default(NbPlanOptions* o) {
    NB_REQUIRE(o, "plan_options_default: null pointer");
    memset(o, 0, sizeof(*o));
    o->conv_mode = NB_CONV_F8;
    // the large split-f16 kernels pay from 128 x 128 output pixels per batch: below ~64 workgroups the fp32 kernels (smaller
    // tiles, split-K) have the lower latency (tools/layers_b1.py: at batch 1 the >= 128x128 layers gain 25-65 %, the <= 64x64
    // layers lose 40-100 %)
    o->h3_min_pixels = 128 * 128;
    o->h3_min_batch = 1;
    o->h3_up2_w16_min_batch = 16;     // 16x16 -> 32x32 conv0 on the large up=2 kernel (8 x 16 quad tiles) from this batch
    o->h3_up2_w8_min_batch = 16;      // 8x8 -> 16x16 likewise (the FIR-folded form on the small-image kernel re-reads 147 KB of
                                      // weights per 32 positions)
    o->small_h3 = o->h2_handoff = o->early_geom_pack = o->fuse_torgb = o->noise_in_kernel = o->positions_once = o->styles_fast = 1;
    return NB_OK;
}

extern "C" int nb_synthesis_plan(const NbGeneratorConfig* cfg, const NbPlanOptions* opts, int n, NbPassPlan* out) {
    NB_REQUIRE(opts, "synthesis_plan: null options");
    GenCfg g;
    const int rc = resolve_cfg(cfg, g);
    return rc ? rc : plan_pass(g, *opts, n, out);
}

extern "C" int nb_generator_param_count(const NbGeneratorConfig* cfg) {
    GenCfg g;
    const int rc = resolve_cfg(cfg, g);
    return rc ? rc : (int)g.params.size();
}

extern "C" int nb_generator_param_info(const NbGeneratorConfig* cfg, int i, char* name, int len, int64_t shape[4], int* ndim) {
    GenCfg g;
    const int rc = resolve_cfg(cfg, g);
    if (rc) return rc;
    NB_REQUIRE(i >= 0 && i < (int)g.params.size(), "generator: parameter index %d out of range [0, %d)", i, (int)g.params.size());
    const GenParam& p = g.params[i];
    if (shape) for (int k = 0; k < 4; ++k) shape[k] = p.shape[k];
    if (ndim) *ndim = p.ndim;
    return copy_name(p.name, name, len);
}

extern "C" int nb_generator_layer_count(const NbGeneratorConfig* cfg, int* num_ws) {
    GenCfg g;
    const int rc = resolve_cfg(cfg, g);
    if (rc) return rc;
    if (num_ws) *num_ws = g.num_ws;
    return (int)g.layers.size();
}

extern "C" int nb_generator_layer_info(const NbGeneratorConfig* cfg, int i, char* name, int len, NbGeneratorLayerInfo* info) {
    GenCfg g;
    const int rc = resolve_cfg(cfg, g);
    if (rc) return rc;
    NB_REQUIRE(i >= 0 && i < (int)g.layers.size(), "generator: layer index %d out of range [0, %d)", i, (int)g.layers.size());
    const GenLayer& l = g.layers[i];
    if (info) *info = NbGeneratorLayerInfo{l.block_res, l.up, l.in_ch, l.out_ch, l.geom_ch, l.w_index};
    return copy_name(l.name, name, len);
}

// ------------------------------------------------------------------------------------------------
// the generator object
// ------------------------------------------------------------------------------------------------

struct GenLayerDev {
    const float *weight = nullptr, *bias = nullptr, *noise_strength = nullptr, *noise_const = nullptr, *affine_w = nullptr,
                *affine_b = nullptr, *filter = nullptr, *noise_grid = nullptr;
    float *wpk = nullptr, *wsq = nullptr, *noise_lin = nullptr, *noise_const_t = nullptr;
    void *w_h3 = nullptr, *w_f8 = nullptr, *w_h3_up2 = nullptr;
    float *styles = nullptr, *dcoefs = nullptr, *noise = nullptr;
};

struct NbGenerator;

// A brush noise set (include/neube_hip.h): per layer noise_const and its transpose in one allocation, and the handle's layer tables
// with noise_const pointing there
struct NbBrushNoise {
    NbGenerator* gen = nullptr;
    float* buf = nullptr;                        // sum over the layers of 2 res^2 floats (each image padded to 256 bytes)
    std::vector<float*> nc, nc_t;                // per layer: [res, res] and its transpose, inside buf
    NbLayerDesc* tables = nullptr;               // as NbGenerator::tables
};

struct NbGenerator {
    GenCfg cfg;
    NbPlanOptions opts;              // nb_plan_options_default with the generator's conv_mode
    int n_max = 0, device = 0;
    float act_gain = 0.f;
    std::vector<void*> allocs;
    std::vector<GenLayerDev> L;
    const float* map_w = nullptr;
    const float* map_b = nullptr;
    const float* w_avg = nullptr;
    const float *trgb_w = nullptr, *trgb_b = nullptr, *trgb_cb = nullptr, *trgb_aw = nullptr, *trgb_ab = nullptr;
    float* trgb_styles = nullptr;
    float* const_rep = nullptr;
    std::vector<NbLayerDesc> host_tables;      // host copy of `tables` (a brush noise set re-points its noise_const)
    NbLayerDesc* tables = nullptr;   // (layers + 1) tables: table k has noise_const cleared for the conv layers >= k (k = layers: full)
    float* ws_buf = nullptr;
    float* npos = nullptr;
    float* act[2] = {nullptr, nullptr};
    void* h2[2] = {nullptr, nullptr};
    std::vector<void*> pre_h2;       // per geometry feature: the consumer's operand tensor its early pack writes (or NULL)
    float *uvs_ws = nullptr, *img_ws = nullptr, *colors_ws = nullptr;
    // workspace sizes (bytes) found by the sizing walk
    size_t need_act = 0, need_h2 = 0;
    std::vector<size_t> need_pre;
    // the geometry encoder (nb_generator_attach_encoder): folded and packed weights, workspaces for every batch up to n_max
    struct Encoder {
        int preproc = -1;                           // NB_GEOM_PREPROC_*; < 0: none attached
        float *w50 = nullptr, *b0 = nullptr;        // the stem: [64][50] folded weights, bias
        void* w_h3[6] = {};                         // the six 3x3 layers: hi/lo f16 weights, f8 weights (f8 generators), bias
        void* w_f8[6] = {};
        float* b[6] = {};
        void* ping[2] = {nullptr, nullptr};         // operand tensors between the layers (the decoder's fp32 output without hand-off)
        float* feat0 = nullptr;                     // the fp32 bottleneck, feature 0
        void* up = nullptr;                         // its bilinear x2 in operand format
        std::vector<void*> allocs;
    } enc;

    NbBrushNoise* brush = nullptr;   // the bound brush noise set (nb_generator_bind_brush_noise), or NULL
    std::vector<NbBrushNoise*> sets; // every live set of this handle (a set that outlives the handle is told so: gen = NULL)

    // bn: the set a constant-noise pass reads its noise_const from (NULL: the checkpoint's)
    const NbLayerDesc* table(int first, const NbBrushNoise* bn = nullptr) const {
        return (bn ? bn->tables : tables) + (size_t)first * (L.size() + 1);
    }
    // the plan of a forward at batch n: constant noise shifted by integer positions, or none; a pass that stops after block
    // stop_res taps that block's fp32 output, one that resumes starts after block resume_res (0 = a whole pass)
    int plan(int n, bool positional, NbPassPlan* p, int stop_res = 0, int resume_res = 0) const {
        NbPlanOptions o = opts;
        o.noise_positions = positional ? NB_PLAN_POS_INT : NB_PLAN_POS_NONE;
        o.tap_mask = stop_res ? 1 << __builtin_ctz(stop_res) : 0;
        o.resume_res = resume_res;
        return plan_pass(cfg, o, n, p);
    }
};

namespace {

size_t h2_bytes(int n, int c, int hw) { return (size_t)n * ((c + 7) / 8) * 2 * hw * 8 * sizeof(_Float16); }

struct WalkSink {
    bool launch = false;                                 // enqueue (else: decisions only)
    bool sizing = false;                                 // record workspace needs (NbGenerator::need_*)
};

#define GEN_TRY(call)                      \
    do {                                   \
        if (sink.launch) {                 \
            const int rc_ = (call);        \
            if (rc_ != NB_OK) return rc_;  \
        }                                  \
    } while (0)

// Runs between the styles and the early geometry packs (SynthesisNetwork._encode_lazy_geometry): fills the geometry inputs and sets
// bit gi of *handed for every feature it wrote into its consumer's operand tensor itself.
using GeomHook = std::function<int(const NbPassPlan&, unsigned* handed)>;

// One forward pass: SynthesisNetwork._prepare + _run_layers for render_triad (constant, seeded or no noise, no feature taps / blending),
// following the pass's plan.  stage (validated by the caller) makes it one half of the painting engine's split: stop_res = the pass of
// `_stop_after` (ends with block stop_res, whose last layer writes stage->features_out; no ToRGB), resume_res = the pass of `_resume`
// (starts behind block resume_res from stage->features_in).
int gen_walk(NbGenerator* g, const NbGeneratorInputs* in, const NbGeneratorOutputs* out, int n, hipStream_t st, const WalkSink& sink,
             const GeomHook* geom_hook = nullptr, const NbGeneratorStage* stage = nullptr) {
    const GenCfg& cfg = g->cfg;
    const std::vector<GenLayer>& specs = cfg.layers;
    const int nL = (int)specs.size(), R = cfg.R, w_dim = cfg.c.w_dim;
    const float clamp = cfg.c.conv_clamp < 0.f ? -1.f : cfg.c.conv_clamp;
    const float alpha = 0.2f, gain = g->act_gain;
    const bool cnoise = in->noise_mode == NB_NOISE_CONST, snoise = in->noise_mode == NB_NOISE_SEEDED;
    const int64_t* ipos = cnoise ? in->positions : nullptr;
    const NbBrushNoise* bn = cnoise ? g->brush : nullptr;      // (the other noise modes ignore a bound set)
    const int stop_res = stage ? stage->stop_res : 0, resume_res = stage ? stage->resume_res : 0;
    const NbGeneratorOutputs no_outputs{};
    if (!out) out = &no_outputs;
    NbPassPlan plan;
    if (const int rc = g->plan(n, ipos != nullptr, &plan, stop_res, resume_res)) return rc;

    // ---- mapping (MappingNetwork.forward) ----
    const float* ws = in->ws;
    if (!ws) {
        GEN_TRY(nb_mapping_ws_f32(in->z, g->map_w, g->map_b, g->ws_buf, n, cfg.c.z_dim, w_dim, cfg.c.mapping_layers,
                                  cfg.c.mapping_lr_multiplier, cfg.num_ws, st));
        if (in->truncation_psi != 1.f && sink.launch) {
            const int cutoff = (in->truncation_cutoff < 0 || in->truncation_cutoff > cfg.num_ws) ? cfg.num_ws : in->truncation_cutoff;
            if (cutoff > 0) {
                hipLaunchKernelGGL(gen_truncate_kernel, dim3(nb_cdiv(n * cutoff * w_dim, 256)), dim3(256), 0, st, g->ws_buf, g->w_avg,
                                   in->truncation_psi, n, cfg.num_ws, w_dim, cutoff);
                NB_CHECK_LAUNCH("generator: truncation");
            }
        }
        ws = g->ws_buf;
    }

    // ---- noise sources (_prepare_noise_sources) ----
    const bool shared = ipos == nullptr;
    const float* npos_k = nullptr;
    if (plan.positions_once) {
        GEN_TRY(nb_norm_positions_f32(ipos, R, g->npos, n, st));
        npos_k = g->npos;
    }
    const int inkernel_from = plan.inkernel_from;      // first layer from which every layer computes its noise itself

    // ---- styles and noise images (_launch_styles_and_noise) ----
    const int n_tab = nL + 1;
    if (plan.styles_noise) {
        GEN_TRY(nb_styles_noise_f32(g->table(inkernel_from < 0 ? nL : inkernel_from, bn), n_tab, ws, cfg.num_ws, w_dim, nullptr, ipos, R, n, st));
    } else {
        GEN_TRY((plan.styles_fast ? nb_styles_fast_f32 : nb_styles_f32)(g->table(nL), n_tab, ws, cfg.num_ws, w_dim, n, st));
        if (cnoise || snoise) {
            // only the layers this pass runs: a head needs no noise image behind its last block, a tail none of the skipped blocks
            int lo = 0, hi = n_tab;
            for (int i = 0; i < nL; ++i) lo += resume_res && specs[i].block_res <= resume_res;
            if (stop_res) {
                hi = 0;
                for (int i = 0; i < nL; ++i) hi += specs[i].block_res <= stop_res;
            }
            if (inkernel_from >= 0) hi = std::min(hi, inkernel_from);      // (constant noise with positions only)
            int max_res = 0;
            for (int i = lo; i < std::min(hi, nL); ++i) max_res = std::max(max_res, specs[i].block_res);
            if (hi > lo && max_res > 0) {
                if (snoise)       // every layer's random image, per sample; the layer index stays absolute in a staged pass
                    GEN_TRY(nb_noise_seeded_f32(g->table(nL) + lo, lo, hi - lo, max_res, in->noise_seed, in->noise_offset, in->noise_state,
                                                n, st));
                else
                    GEN_TRY(nb_noise_f32(g->table(nL, bn) + lo, hi - lo, max_res, npos_k, npos_k ? nullptr : ipos, R, n, st));
            }
        }
    }

    // ---- geometry from stroke patches (_encode_lazy_geometry) ----
    unsigned handed = 0;
    if (geom_hook && sink.launch)
        if (const int rc = (*geom_hook)(plan, &handed)) return rc;

    // ---- early geometry packs (_pack_geometry_early; in-line on the one stream) ----
    const int ng = (int)cfg.geom_res.size();
    for (int gi = 0; gi < ng; ++gi) {
        const NbGeomPlan& gp = plan.geom[gi];
        if (!gp.early_pack || ((handed >> gi) & 1)) continue;
        const int gres = cfg.geom_res[gi], gch = cfg.geom_ch[gi], ic = gp.consumer;
        const GenLayer& sc = specs[ic];
        if (sink.sizing) g->need_pre[gi] = std::max(g->need_pre[gi], h2_bytes(n, sc.in_ch, gres * gres));
        const int c_prod = sc.in_ch - gch;
        GEN_TRY((gp.fmt ? nb_pack_h2f8_part_f32 : nb_pack_h2_part_f32)(in->geom[gi], gch, g->L[ic].styles + c_prod, sc.in_ch, g->pre_h2[gi],
                                                                       (sc.in_ch + 7) / 8, c_prod / 8, n, gres * gres, st));
    }

    // ---- the layers (_run_layers / _run_layer / _finish_block) ----
    const float* x = resume_res ? nullptr : g->const_rep;       // fp32 NCHW input of the next layer (NULL: handed over in operand format)
    int xc = cfg.channels(4);
    const float* x2 = nullptr;                        // geometry feature still to be concatenated
    int x2c = 0;
    void* xh2 = nullptr;                              // the next layer's complete operand-format input, when its producer wrote it
    float* uvs = out->uvs ? out->uvs : g->uvs_ws;
    float* img = out->img ? out->img : g->img_ws;
    float* colors = out->colors ? out->colors : g->colors_ws;
    const int c_last = cfg.channels(R);
    int geo_idx = 0;
    auto other_act = [&](const float* cur) { return cur == g->act[0] ? g->act[1] : g->act[0]; };
    auto other_h2 = [&](const void* cur) { return cur == g->h2[0] ? g->h2[1] : g->h2[0]; };
    for (int i = 0; i < nL; ++i) {
        const GenLayer& s = specs[i];
        const GenLayerDev& d = g->L[i];
        const NbLayerPlan& lp = plan.layers[i];
        const int res = s.block_res, ir = s.in_res();
        if (resume_res && res <= resume_res) {
            // a block the resumed pass skips (_run_layers): its output is the caller's, and the geometry index moves on
            if (s.up == 1 && res == resume_res) {
                x = stage->features_in;
                xc = s.out_ch;
            }
            if (s.up == 1 && cfg.geom_index(res) >= 0) {
                if (res == resume_res) {
                    x2 = in->geom[geo_idx];
                    x2c = cfg.geom_ch[geo_idx];
                }
                ++geo_idx;
            }
            continue;
        }
        const int c2 = x2c;                           // (not the pointer: the sizing walk carries none)
        const int c1 = x ? xc : s.in_ch - c2;
        if (c1 + c2 != s.in_ch) {
            nb_set_error("generator: %s got %d+%d input channels, expected %d", s.name.c_str(), c1, c2, s.in_ch);
            return NB_EINVAL;
        }
        NbNoiseSrc nsrc{};
        const float* noise = nullptr;
        int64_t nstride = 0;
        if (lp.noise_in_kernel) {
            nsrc = NbNoiseSrc{bn ? bn->nc_t[i] : d.noise_const_t, d.noise_lin, d.noise_strength, npos_k, npos_k ? nullptr : ipos, res, R};
            noise = (const float*)&nsrc;
            nstride = NB_NOISE_IN_KERNEL;
        } else if (cnoise || snoise) {
            noise = d.noise;
            nstride = (cnoise && shared) ? 0 : (int64_t)res * res;
        }
        const bool is_last = res == R;
        const bool head_last = stop_res && s.up == 1 && res == stop_res;      // the tapped layer: fp32 into the caller's buffer
        const bool fused_torgb = lp.fused_torgb && !head_last;
        const int gi_after = s.up == 1 ? cfg.geom_index(res) : -1;
        float* y = nullptr;
        void* next_h2 = nullptr;
        if (lp.kind == NB_KERNEL_LARGE_H3) {
            const void* wts = lp.in_fmt ? d.w_f8 : d.w_h3;
            if (!wts) {                                 // (at creation the sizing walk stops here: nb_generator_create fails)
                nb_set_error("generator: %s has no packed weights for operand format %d", s.name.c_str(), lp.in_fmt);
                return NB_EINVAL;
            }
            if (!xh2) {                                 // producer was not a split-f16 kernel: (x ++ geometry) * styles -> operands
                xh2 = g->h2[0];
                if (sink.sizing) g->need_h2 = std::max(g->need_h2, h2_bytes(n, s.in_ch, ir * ir));
                GEN_TRY((lp.in_fmt ? nb_pack_h2f8_f32 : nb_pack_h2_f32)(x, c1, x2, c2, d.styles, xh2, n, ir * ir, st));
            }
            NbTorgbArgs targs{};
            if (fused_torgb) {
                targs = NbTorgbArgs{g->trgb_styles, g->trgb_w, g->trgb_b, g->trgb_cb, nullptr, uvs, img, colors, in->user_colors,
                                    in->sfactor, out->rgba, out->rgba_u8, s.out_ch + 9, in->render_mode, clamp};
            } else if (lp.handoff) {
                if (gi_after >= 0 && plan.geom[gi_after].early_pack) {
                    next_h2 = g->pre_h2[gi_after];
                } else {
                    next_h2 = other_h2(xh2);
                    if (sink.sizing) g->need_h2 = std::max(g->need_h2, h2_bytes(n, specs[i + 1].in_ch, res * res));
                }
            } else if (head_last) {
                y = stage->features_out;
            } else {
                y = other_act(x);
                if (sink.sizing) g->need_act = std::max(g->need_act, (size_t)n * s.out_ch * res * res * sizeof(float));
            }
            const float* nst = next_h2 ? g->L[i + 1].styles : nullptr;
            const int c_next = next_h2 ? specs[i + 1].in_ch : 0;
            if (s.up == 1) {
                GEN_TRY(nb_modconv3x3_up1_h3_ex(xh2, s.in_ch, wts, d.dcoefs, noise, nstride, d.bias, y, next_h2, nst, c_next, c_next,
                                                fused_torgb ? &targs : nullptr, lp.kernel_fmt, lp.out_fmt, n, ir, ir, s.out_ch, alpha,
                                                gain, clamp, st));
            } else {
                GEN_TRY(nb_modconv3x3_up2_h3_ex(xh2, s.in_ch, wts, d.dcoefs, noise, nstride, d.bias, y, next_h2, nst, c_next, c_next,
                                                lp.kernel_fmt, lp.out_fmt, n, ir, ir, s.out_ch, alpha, gain, clamp, st));
            }
        } else {
            y = head_last ? stage->features_out : other_act(x);
            if (sink.sizing && !head_last) g->need_act = std::max(g->need_act, (size_t)n * s.out_ch * res * res * sizeof(float));
            if (lp.kind == NB_KERNEL_SMALL_H3 && s.up == 1) {
                GEN_TRY(nb_modconv3x3_up1_small_h3(x, c1, d.w_h3, d.styles, d.dcoefs, noise, nstride, d.bias, y, n, ir, ir, s.out_ch,
                                                   alpha, gain, clamp, st));
            } else if (lp.kind == NB_KERNEL_SMALL_H3) {
                GEN_TRY(nb_modconv3x3_up2_small_h3(x, c1, x2, c2, d.w_h3_up2, d.styles, d.dcoefs, noise, nstride, d.bias, y, n, ir, ir,
                                                   s.out_ch, alpha, gain, clamp, st));
            } else {
                GEN_TRY(nb_modconv3x3_f32(x, c1, x2, c2, d.wpk, d.styles, d.dcoefs, noise, nstride, d.bias, y, n, ir, ir, s.out_ch, s.up,
                                          alpha, gain, clamp, st));
            }
        }
        xh2 = next_h2;
        x = y;
        xc = s.out_ch;
        x2 = nullptr;
        x2c = 0;
        if (head_last) return NB_OK;                  // (_stop_after: no ToRGB, no geometry behind the block)
        if (s.up == 2) continue;
        // ---- what follows a block's last layer ----
        if (is_last && !fused_torgb) {
            GEN_TRY(nb_torgb_triad_f32(x, g->trgb_styles, c_last + 9, g->trgb_w, g->trgb_b, g->trgb_cb, clamp, nullptr, uvs, img, colors,
                                       in->user_colors, in->sfactor, in->render_mode, out->rgba, out->rgba_u8, n, c_last, R * R, st));
        }
        if (gi_after < 0) continue;
        const float* gf = in->geom[geo_idx];
        const int gch = cfg.geom_ch[geo_idx];
        if (xh2 && plan.geom[geo_idx].early_pack && xh2 == g->pre_h2[geo_idx]) {
            // packed at the start of the pass
        } else if (xh2) {
            // the block's last layer wrote its channels into the consumer's operands: the geometry channels go behind them
            const GenLayer& sn = specs[i + 1];
            const int c_prod = sn.in_ch - gch;
            GEN_TRY((plan.layers[i + 1].in_fmt ? nb_pack_h2f8_part_f32 : nb_pack_h2_part_f32)(gf, gch, g->L[i + 1].styles + c_prod, sn.in_ch,
                                                                                              xh2, (sn.in_ch + 7) / 8, c_prod / 8, n, res * res, st));
        } else {
            x2 = gf;
            x2c = gch;
        }
        ++geo_idx;
    }
    if (resume_res == R) {                            // resumed behind the last block: nothing but its ToRGB is left
        GEN_TRY(nb_torgb_triad_f32(stage->features_in, g->trgb_styles, c_last + 9, g->trgb_w, g->trgb_b, g->trgb_cb, clamp, nullptr, uvs, img,
                                   colors, in->user_colors, in->sfactor, in->render_mode, out->rgba, out->rgba_u8, n, c_last, R * R, st));
    }
    return NB_OK;
}

#undef GEN_TRY

void gen_free(NbGenerator* g) {
    if (!g) return;
    for (NbBrushNoise* s : g->sets) s->gen = nullptr;
    int prev = 0;
    const bool have = hipGetDevice(&prev) == hipSuccess;
    if ((!g->allocs.empty() || !g->enc.allocs.empty()) && hipSetDevice(g->device) == hipSuccess) {
        (void)hipDeviceSynchronize();
        for (void* p : g->allocs) (void)hipFree(p);
        for (void* p : g->enc.allocs) (void)hipFree(p);
    }
    if (have) (void)hipSetDevice(prev);
    delete g;
}

}  // namespace

extern "C" int nb_generator_destroy(NbGenerator* gen) {
    gen_free(gen);
    return NB_OK;
}

extern "C" int nb_generator_create(const NbGeneratorConfig* cfg, const void* const* params_dev, int conv_mode, int n_max, void* stream,
                                   NbGenerator** out) {
    NB_REQUIRE(out, "generator_create: null output handle");
    *out = nullptr;
    GenCfg gc;
    int rc = resolve_cfg(cfg, gc);
    if (rc) return rc;
    if (conv_mode == NB_CONV_F6 || conv_mode == NB_CONV_F16) {
        nb_set_error("generator_create: conv_mode %d (f6 / f16) is not supported by the C entry (f32, h3, f8 are)", conv_mode);
        return NB_EUNSUPPORTED;
    }
    if (conv_mode != NB_CONV_F32 && conv_mode != NB_CONV_H3 && conv_mode != NB_CONV_F8) {
        nb_set_error("generator_create: unknown conv_mode %d", conv_mode);
        return NB_EUNSUPPORTED;
    }
    NB_REQUIRE(n_max >= 1 && n_max <= 65535, "generator_create: n_max must be in [1, 65535]");
    NB_REQUIRE(params_dev, "generator_create: null parameter array");
    for (size_t i = 0; i < gc.params.size(); ++i)
        NB_REQUIRE(params_dev[i], "generator_create: parameter %d (%s) is NULL", (int)i, gc.params[i].name.c_str());

    NbGenerator* g = new NbGenerator();
    g->cfg = gc;
    nb_plan_options_default(&g->opts);
    g->opts.conv_mode = conv_mode;
    g->n_max = n_max;
    g->act_gain = (float)std::sqrt(2.0);
    hipStream_t st = (hipStream_t)stream;
    if (hipGetDevice(&g->device) != hipSuccess) {
        delete g;
        nb_set_error("generator_create: no HIP device");
        return NB_ELAUNCH;
    }
    const GenCfg& C = g->cfg;
    const int nL = (int)C.layers.size(), w_dim = C.c.w_dim;
    bool ok = true;
    auto alloc = [&](size_t bytes) -> void* {
        void* p = nullptr;
        if (!ok || bytes == 0) return nullptr;
        if (hipMalloc(&p, (bytes + 255) / 256 * 256) != hipSuccess) {
            ok = false;
            nb_set_error("generator_create: hipMalloc of %zu bytes failed", bytes);
            return nullptr;
        }
        g->allocs.push_back(p);
        return p;
    };
    auto launched = [&]() -> int {
        NB_CHECK_LAUNCH("generator_create");
        return NB_OK;
    };
    auto fail = [&](int code) {
        gen_free(g);
        return code;
    };
    // the caller's parameters, copied (they may be freed after this call)
    std::vector<const float*> P(C.params.size());
    for (size_t i = 0; i < C.params.size(); ++i) {
        const size_t bytes = (size_t)C.params[i].numel() * sizeof(float);
        float* p = (float*)alloc(bytes);
        if (!ok) return fail(NB_ELAUNCH);
        if (hipMemcpyAsync(p, params_dev[i], bytes, hipMemcpyDeviceToDevice, st) != hipSuccess) {
            nb_set_error("generator_create: copy of parameter %s failed", C.params[i].name.c_str());
            return fail(NB_ELAUNCH);
        }
        P[i] = p;
    }
    int pi = 0;
    // mapping: the FC weights / biases concatenated (MappingNetwork._pack)
    {
        size_t wn = 0;
        for (int i = 0; i < C.c.mapping_layers; ++i) wn += (size_t)C.params[2 * i].numel();
        float* mw = (float*)alloc(wn * sizeof(float));
        float* mb = (float*)alloc((size_t)C.c.mapping_layers * w_dim * sizeof(float));
        if (!ok) return fail(NB_ELAUNCH);
        size_t off = 0;
        for (int i = 0; i < C.c.mapping_layers; ++i) {
            const size_t k = (size_t)C.params[2 * i].numel();
            bool copied = hipMemcpyAsync(mw + off, P[2 * i], k * sizeof(float), hipMemcpyDeviceToDevice, st) == hipSuccess;
            copied = copied && hipMemcpyAsync(mb + (size_t)i * w_dim, P[2 * i + 1], w_dim * sizeof(float), hipMemcpyDeviceToDevice, st) == hipSuccess;
            if (!copied) {
                nb_set_error("generator_create: copy of the mapping weights failed");
                return fail(NB_ELAUNCH);
            }
            off += k;
        }
        g->map_w = mw;
        g->map_b = mb;
        pi = 2 * C.c.mapping_layers;
    }
    g->w_avg = P[pi++];
    const float* b4_const = P[pi++];
    pi += (int)C.blocks.size();                        // the blocks' resample filters (the layers carry their own)
    const int c4 = C.channels(4);
    g->const_rep = (float*)alloc((size_t)n_max * c4 * 16 * sizeof(float));
    if (!ok) return fail(NB_ELAUNCH);
    hipLaunchKernelGGL(gen_repeat_kernel, dim3(nb_cdiv(n_max * c4 * 16, 256)), dim3(256), 0, st, b4_const, c4 * 16, n_max, g->const_rep);
    if ((rc = launched())) return fail(rc);
    NbPassPlan plan;                                   // (the weight forms a layer needs do not depend on the batch)
    if ((rc = g->plan(1, true, &plan))) return fail(rc);
    g->L.resize(nL);
    for (int i = 0; i < nL; ++i) {
        const GenLayer& s = C.layers[i];
        GenLayerDev& d = g->L[i];
        const int packs = plan.layers[i].packs;
        d.weight = P[pi++]; d.noise_strength = P[pi++]; d.bias = P[pi++]; d.noise_grid = P[pi++]; d.filter = P[pi++];
        d.noise_const = P[pi++]; d.affine_w = P[pi++]; d.affine_b = P[pi++];
        const int r = s.block_res;
        d.wpk = (float*)alloc((size_t)(s.in_ch + 7) / 8 * 8 * 9 * ((s.out_ch + 31) / 32 * 32) * sizeof(float));
        d.wsq = (float*)alloc((size_t)s.in_ch * s.out_ch * sizeof(float));
        d.noise_lin = (float*)alloc((size_t)r * sizeof(float));
        d.noise_const_t = (float*)alloc((size_t)r * r * sizeof(float));
        d.styles = (float*)alloc((size_t)n_max * s.in_ch * sizeof(float));
        d.dcoefs = (float*)alloc((size_t)n_max * s.out_ch * sizeof(float));
        d.noise = (float*)alloc((size_t)n_max * r * r * sizeof(float));
        const size_t h3_bytes = (size_t)(s.in_ch + 15) / 16 * 9 * 4 * ((s.out_ch + 63) / 64 * 64) * 8 * sizeof(_Float16);
        if (packs & NB_PACK_H3) d.w_h3 = alloc(h3_bytes);
        if (packs & NB_PACK_F8) d.w_f8 = alloc(h3_bytes);
        if (packs & NB_PACK_H3_UP2) d.w_h3_up2 = alloc(4 * h3_bytes);
        if (!ok) return fail(NB_ELAUNCH);
        if ((rc = nb_pack_conv_weight_dev(d.weight, s.out_ch, s.in_ch, d.wpk, d.wsq, st))) return fail(rc);
        if (d.w_h3 && (rc = nb_pack_conv_weight_h3_dev(d.weight, s.out_ch, s.in_ch, 64, 0, d.w_h3, st))) return fail(rc);
        if (d.w_f8 && (rc = nb_pack_conv_weight_h3f8_dev(d.weight, s.out_ch, s.in_ch, d.w_f8, st))) return fail(rc);
        if (d.w_h3_up2 && (rc = nb_pack_conv_weight_h3_up2_dev(d.weight, d.filter, s.out_ch, s.in_ch, d.w_h3_up2, st))) return fail(rc);
        hipLaunchKernelGGL(gen_gather_kernel, dim3(nb_cdiv(r, 256)), dim3(256), 0, st, d.noise_grid, 2 * r, r, d.noise_lin);
        hipLaunchKernelGGL(gen_transpose_kernel, dim3(nb_cdiv(r * r, 256)), dim3(256), 0, st, d.noise_const, r, d.noise_const_t);
        if ((rc = launched())) return fail(rc);
    }
    g->trgb_w = P[pi++]; g->trgb_b = P[pi++]; g->trgb_cb = P[pi++]; g->trgb_aw = P[pi++]; g->trgb_ab = P[pi++];
    const int c_last = C.channels(C.R);
    g->trgb_styles = (float*)alloc((size_t)n_max * (c_last + 9) * sizeof(float));
    // layer tables (_Plan): the full one and, for the fused styles + noise launch of small batches, one per first in-kernel-noise layer
    std::vector<NbLayerDesc>& descs = g->host_tables;
    descs.resize((size_t)(nL + 1) * (nL + 1));
    for (int first = 0; first <= nL; ++first) {
        NbLayerDesc* t = descs.data() + (size_t)first * (nL + 1);
        for (int i = 0; i < nL; ++i) {
            const GenLayer& s = C.layers[i];
            const GenLayerDev& d = g->L[i];
            t[i] = NbLayerDesc{d.affine_w, d.affine_b, d.wsq, d.styles, d.dcoefs, i >= first ? nullptr : d.noise_const, d.noise_lin, d.noise,
                               d.noise_strength, s.in_ch, 0, s.out_ch, s.w_index, s.block_res, 1.f, {0, 0}};
        }
        t[nL] = NbLayerDesc{g->trgb_aw, g->trgb_ab, nullptr, g->trgb_styles, nullptr, nullptr, nullptr, nullptr, nullptr, c_last + 9, 9, 3,
                            nL, 0, (float)(1.0 / std::sqrt((double)c_last)), {0, 0}};
    }
    g->tables = (NbLayerDesc*)alloc(descs.size() * sizeof(NbLayerDesc));
    g->ws_buf = (float*)alloc((size_t)n_max * C.num_ws * w_dim * sizeof(float));
    g->npos = (float*)alloc((size_t)n_max * 2 * sizeof(float));
    g->uvs_ws = (float*)alloc((size_t)n_max * 3 * C.R * C.R * sizeof(float));
    g->img_ws = (float*)alloc((size_t)n_max * 3 * C.R * C.R * sizeof(float));
    g->colors_ws = (float*)alloc((size_t)n_max * 9 * sizeof(float));
    if (!ok) return fail(NB_ELAUNCH);
    if (hipMemcpyAsync(g->tables, descs.data(), descs.size() * sizeof(NbLayerDesc), hipMemcpyHostToDevice, st) != hipSuccess) {
        nb_set_error("generator_create: upload of the layer tables failed");
        return fail(NB_ELAUNCH);
    }
    // workspaces: the largest each buffer gets at any batch size up to n_max (decisions change with the batch)
    {
        static char sentinel[8];
        g->act[0] = (float*)&sentinel[0]; g->act[1] = (float*)&sentinel[2];
        g->h2[0] = &sentinel[4]; g->h2[1] = &sentinel[6];
        g->pre_h2.assign(C.geom_res.size(), nullptr);
        g->need_pre.assign(C.geom_res.size(), 0);
        for (size_t k = 0; k < C.geom_res.size(); ++k) g->pre_h2[k] = &sentinel[1];
        NbGeneratorInputs din{};
        din.z = (const float*)&sentinel[3];
        din.positions = (const int64_t*)&sentinel[5];
        din.truncation_psi = 1.f;
        NbGeneratorOutputs dout{};
        WalkSink sink;
        sink.sizing = true;
        for (int n = 1; n <= n_max; ++n)
            if ((rc = gen_walk(g, &din, &dout, n, st, sink))) return fail(rc);
        // ... and every stage of nb_generator_forward_staged: a resumed pass packs the caller's fp32 features where a whole pass hands
        // operands over (or packs them early into a tensor of its own); a head's tapped layer writes into the caller's buffer
        for (int res : C.blocks)
            for (int half = 0; half < 2; ++half) {
                NbGeneratorStage sg{};
                (half ? sg.resume_res : sg.stop_res) = res;
                sg.features_out = (float*)&sentinel[7];
                sg.features_in = (const float*)&sentinel[7];
                for (int n = 1; n <= n_max; ++n)
                    if ((rc = gen_walk(g, &din, &dout, n, st, sink, nullptr, &sg))) return fail(rc);
            }
        g->act[0] = (float*)alloc(g->need_act); g->act[1] = (float*)alloc(g->need_act);
        g->h2[0] = alloc(g->need_h2); g->h2[1] = alloc(g->need_h2);
        for (size_t k = 0; k < C.geom_res.size(); ++k) g->pre_h2[k] = alloc(g->need_pre[k]);
        if (!ok) return fail(NB_ELAUNCH);
    }
    if (hipStreamSynchronize(st) != hipSuccess) {
        nb_set_error("generator_create: %s", hipGetErrorString(hipGetLastError()));
        return fail(NB_ELAUNCH);
    }
    *out = g;
    return NB_OK;
}

namespace {

// the input rules of a forward pass (`who` prefixes the messages); the geometry features are checked by the caller
int check_forward(NbGenerator* gen, const NbGeneratorInputs* in, int n, void* stream, const char* who) {
    NB_REQUIRE(n >= 1 && n <= gen->n_max, "%s: batch %d outside [1, n_max = %d]", who, n, gen->n_max);
    NB_REQUIRE((in->z != nullptr) != (in->ws != nullptr), "%s: pass exactly one of z / ws", who);
    NB_REQUIRE(in->truncation_psi == 1.f || in->z, "%s: truncation applies to z input only (ws input needs psi = 1)", who);
    return NB_OK;
}

int check_modes_and_device(NbGenerator* gen, const NbGeneratorInputs* in, void* stream, const char* who) {
    if (in->noise_mode != NB_NOISE_CONST && in->noise_mode != NB_NOISE_NONE && in->noise_mode != NB_NOISE_SEEDED) {
        nb_set_error("%s: noise_mode %d not supported (const and none are)", who, in->noise_mode);
        return in->noise_mode == NB_NOISE_RANDOM ? NB_EUNSUPPORTED : NB_EINVAL;
    }
    NB_REQUIRE(in->render_mode == NB_RENDER_CLEAR || in->render_mode == NB_RENDER_FULL, "%s: unknown render_mode %d", who, in->render_mode);
    int dev = -1;
    NB_REQUIRE(hipGetDevice(&dev) == hipSuccess && dev == gen->device, "%s: current device %d is not the generator's (%d)", who, dev,
               gen->device);
    if (stream) {
        hipDevice_t sdev = -1;
        NB_REQUIRE(hipStreamGetDevice((hipStream_t)stream, &sdev) == hipSuccess && sdev == gen->device,
                   "%s: the stream belongs to device %d, the generator to %d", who, (int)sdev, gen->device);
    }
    return NB_OK;
}

}  // namespace

extern "C" int nb_generator_forward(NbGenerator* gen, const NbGeneratorInputs* in, const NbGeneratorOutputs* out, int n, void* stream) {
    NB_REQUIRE(gen && in && out, "generator_forward: null pointer");
    if (const int rc = check_forward(gen, in, n, stream, "generator_forward")) return rc;
    for (size_t k = 0; k < gen->cfg.geom_res.size(); ++k) NB_REQUIRE(in->geom[k], "generator_forward: geometry feature %d is NULL", (int)k);
    if (const int rc = check_modes_and_device(gen, in, stream, "generator_forward")) return rc;
    WalkSink sink;
    sink.launch = true;
    return gen_walk(gen, in, out, n, (hipStream_t)stream, sink);
}

extern "C" int nb_generator_describe(NbGenerator* gen, int n, char* buf, int len) {
    NB_REQUIRE(gen && buf && len > 0, "generator_describe: bad arguments");
    NB_REQUIRE(n >= 1 && n <= gen->n_max, "generator_describe: batch %d outside [1, n_max = %d]", n, gen->n_max);
    NbPassPlan plan;
    if (const int rc = gen->plan(n, true, &plan)) return rc;
    std::string s;
    for (int i = 0; i < plan.num_layers; ++i) s += gen->cfg.layers[i].name + "=" + plan.layers[i].kernel + "\n";
    const NbLayerPlan& last = plan.layers[plan.num_layers - 1];
    s += fmt("synthesis.b%d.torgb=", gen->cfg.R) + (last.fused_torgb ? last.kernel : "torgb_triad_kernel") + "\n";
    NB_REQUIRE(len > (int)s.size(), "generator_describe: buffer of %d bytes, %d needed", len, (int)s.size() + 1);
    memcpy(buf, s.c_str(), s.size() + 1);
    return NB_OK;
}

// ------------------------------------------------------------------------------------------------
// the geometry encoder behind the generator handle: stroke patches -> the two features (encoder.HipGeometryEncoder.encode, driven
// as SynthesisNetwork._encode_lazy_geometry drives it)
// ------------------------------------------------------------------------------------------------
namespace {

struct EncLayer {
    const char* prefix;
    int c_out, c_in, k, stride;
};
// the stem, then the six 3x3 layers of HipGeometryEncoder.convs: three stride-2 stages, 256 -> 32 -> 16 (the bottleneck) and the first
// decoder stage (behind the bilinear x2)
const EncLayer kEncLayers[7] = {{"encoder.model.0.conv", 64, 1, 7, 1},   {"encoder.model.1.conv", 128, 64, 3, 2},
                                {"encoder.model.2.conv", 256, 128, 3, 2}, {"encoder.model.3.conv", 256, 256, 3, 2},
                                {"encoder.model.4.conv", 32, 256, 3, 1},  {"encoder.model.5.conv", 16, 32, 3, 1},
                                {"decoder.model.0.conv.conv", 256, 16, 3, 1}};
constexpr int kEncParamsPerLayer = 6;             // conv weight, conv bias, BatchNorm weight, bias, running mean, running var

std::vector<GenParam> enc_params() {
    std::vector<GenParam> v;
    GenCfg tmp;
    for (const EncLayer& L : kEncLayers) {
        const std::string p = L.prefix;
        add_param(tmp, p + ".0.weight", {L.c_out, L.c_in, L.k, L.k});
        add_param(tmp, p + ".0.bias", {L.c_out});
        add_param(tmp, p + ".1.weight", {L.c_out});
        add_param(tmp, p + ".1.bias", {L.c_out});
        add_param(tmp, p + ".1.running_mean", {L.c_out});
        add_param(tmp, p + ".1.running_var", {L.c_out});
    }
    return tmp.params;
}

// can an encoder be attached to a generator of this configuration?
int enc_check(const GenCfg& g, int preproc, const char* who) {
    const int R = g.R;
    NB_REQUIRE(g.geom_res.size() == 2 && g.geom_ch[0] == 16 && g.geom_ch[1] == 256 && g.geom_res[0] == R / 8 && g.geom_res[1] == R / 4,
               "%s: the generator's geometry layout is not the encoder's (two features: 16 channels at R/8, 256 at R/4)", who);
    NB_REQUIRE(R == 32 || R == 64 || (R >= 128 && R % 128 == 0), "%s: patch size %d is not one the encoder tiles (32, 64 or a multiple of 128)",
               who, R);
    NB_REQUIRE(preproc >= NB_GEOM_PREPROC_NONE && preproc <= NB_GEOM_PREPROC_INVERSE, "%s: unknown preproc %d", who, preproc);
    return NB_OK;
}

// Operand format between the encoder's layers at batch n (HipGeometryEncoder.encode with TileOps' rule arith = "f8" iff the generator
// is f8): "f8" from batch 8 at patch sizes the large tiles cover, else H2 (the small-tile kernels of interactive strokes read H2)
int enc_fmt(const NbGenerator* g, int n) {
    const int R = g->cfg.R;
    return g->opts.conv_mode == NB_CONV_F8 && n >= 8 && R >= 128 && R % 128 == 0;
}

// HipGeometryEncoder.encode on the handle's workspaces.  launch = false: record the largest ping-pong tensor in *need_ping only.
// Otherwise io->geom[] receives the fp32 features, and feature 1 goes straight into its consumer's operand tensor (pre_h2[1], times
// the consumer's styles) where the plan's encoder hand-off and the patch size allow it: bit 1 of *handed is then set.
int enc_walk(NbGenerator* g, const float* x, int n, hipStream_t st, const NbPassPlan* plan, bool launch, size_t* need_ping,
             NbGeneratorInputs* io, unsigned* handed) {
    const NbGenerator::Encoder& E = g->enc;
    const int R = g->cfg.R;
    const float slope = 0.01f;
    const int fmt = enc_fmt(g, n);
    const bool fused = fmt && R % 64 == 0;          // stem + first stride-2 stage in one launch (NB_ENC_FUSE_STEM's default)
    // the 3x3 layers with <= 32 outputs from >= 32 inputs run on the split-K tiles, which read H2: their producers write H2
    auto narrow = [](int i) { return kEncLayers[i + 1].c_out <= 32 && kEncLayers[i + 1].c_in >= 32; };
    auto W = [&](int i, int f) -> const void* { return f ? E.w_f8[i] : E.w_h3[i]; };
    auto need = [&](size_t b) {
        if (need_ping) *need_ping = std::max(*need_ping, b);
    };
#define ENC_TRY(call)                     \
    do {                                  \
        if (launch) {                     \
            const int rc_ = (call);       \
            if (rc_ != NB_OK) return rc_; \
        }                                 \
    } while (0)
    int cur = 0, r = R;
    if (fused) {
        need(h2_bytes(n, kEncLayers[1].c_out, (R / 2) * (R / 2)));
        ENC_TRY(nb_enc_stem_conv3x3_f8(x, E.w50, E.b0, E.preproc, W(0, 1), E.b[0], E.ping[0], narrow(1) ? 0 : fmt, n, R, R,
                                       kEncLayers[1].c_out, slope, st));
        r = R / 2;
    } else {
        need(h2_bytes(n, kEncLayers[0].c_out, R * R));
        ENC_TRY(nb_enc_stem7x7_f32_h2_ex(x, E.w50, E.b0, E.ping[0], fmt, n, R, R, E.preproc, slope, st));
    }
    for (int i = fused ? 1 : 0; i < 4; ++i) {       // three stride-2 stages + 256 -> 32
        const EncLayer& L = kEncLayers[i + 1];
        const int ro = r / L.stride, fin = narrow(i) ? 0 : fmt, fout = narrow(i + 1) ? 0 : fmt;
        need(h2_bytes(n, L.c_out, ro * ro));
        ENC_TRY(nb_enc_conv3x3_ex(E.ping[cur], L.c_in, W(i, fin), E.b[i], nullptr, E.ping[cur ^ 1], nullptr, 0, fout ? L.c_out / 8 : 0, 0, fin,
                                  fout, n, r, r, L.c_out, L.stride, slope, st));
        cur ^= 1;
        r = ro;
    }
    const EncLayer& B = kEncLayers[5];              // 32 -> 16: the bottleneck, feature 0 (fp32)
    const int fin = narrow(4) ? 0 : fmt;
    ENC_TRY(nb_enc_conv3x3_ex(E.ping[cur], B.c_in, W(4, fin), E.b[4], E.feat0, nullptr, nullptr, 0, 0, 0, fin, 0, n, r, r, B.c_out, 1, slope, st));
    ENC_TRY(nb_enc_upsample2x_h2_ex(E.feat0, E.up, fmt, n, B.c_out, r, r, st));
    const EncLayer& D = kEncLayers[6];              // the first decoder stage, 16 -> 256: feature 1
    const int r1 = 2 * r;
    need((size_t)n * D.c_out * r1 * r1 * sizeof(float));
    if (!launch) return NB_OK;
    io->geom[0] = E.feat0;
    const NbGeomPlan& gp = plan->geom[1];
    // the hand-off needs the large-tile epilogue (HipGeometryEncoder.can_handoff) and the consumer's operand tensor of the early pack
    if (gp.encoder_handoff && gp.early_pack && (r1 % 32 == 0 || r1 == 16)) {
        const GenLayer& sc = g->cfg.layers[gp.consumer];
        const int c_prod = sc.in_ch - D.c_out;
        ENC_TRY(nb_enc_conv3x3_ex(g->enc.up, D.c_in, W(5, fmt), E.b[5], nullptr, g->pre_h2[1], g->L[gp.consumer].styles + c_prod, sc.in_ch,
                                  sc.in_ch / 8, c_prod / 8, fmt, gp.fmt, n, r1, r1, D.c_out, 1, slope, st));
        io->geom[1] = nullptr;
        *handed |= 2u;
    } else {
        float* dec = (float*)E.ping[cur ^ 1];
        ENC_TRY(nb_enc_conv3x3_ex(E.up, D.c_in, W(5, fmt), E.b[5], dec, nullptr, nullptr, 0, 0, 0, fmt, 0, n, r1, r1, D.c_out, 1, slope, st));
        io->geom[1] = dec;
    }
#undef ENC_TRY
    return NB_OK;
}

void enc_free(NbGenerator* g) {
    if (!g->enc.allocs.empty()) {
        (void)hipDeviceSynchronize();
        for (void* p : g->enc.allocs) (void)hipFree(p);
    }
    g->enc = NbGenerator::Encoder();
}

}  // namespace

extern "C" int nb_encoder_param_count(void) { return (int)(sizeof(kEncLayers) / sizeof(kEncLayers[0])) * kEncParamsPerLayer; }

extern "C" int nb_encoder_param_info(int i, char* name, int len, int64_t shape[4], int* ndim) {
    const std::vector<GenParam> ps = enc_params();
    NB_REQUIRE(i >= 0 && i < (int)ps.size(), "encoder: parameter index %d out of range [0, %d)", i, (int)ps.size());
    const GenParam& p = ps[i];
    if (shape) for (int k = 0; k < 4; ++k) shape[k] = p.shape[k];
    if (ndim) *ndim = p.ndim;
    return copy_name(p.name, name, len);
}

extern "C" int nb_generator_encoder_check(const NbGeneratorConfig* cfg, int preproc) {
    GenCfg g;
    const int rc = resolve_cfg(cfg, g);
    return rc ? rc : enc_check(g, preproc, "encoder_check");
}

extern "C" int nb_generator_attach_encoder(NbGenerator* gen, const void* const* enc_params_dev, int preproc, void* stream) {
    NB_REQUIRE(gen, "generator_attach_encoder: null generator");
    if (const int rc = enc_check(gen->cfg, preproc, "generator_attach_encoder")) return rc;
    NB_REQUIRE(enc_params_dev, "generator_attach_encoder: null parameter array");
    const std::vector<GenParam> ps = enc_params();
    for (size_t i = 0; i < ps.size(); ++i)
        NB_REQUIRE(enc_params_dev[i], "generator_attach_encoder: parameter %d (%s) is NULL", (int)i, ps[i].name.c_str());
    int dev = -1;
    NB_REQUIRE(hipGetDevice(&dev) == hipSuccess && dev == gen->device, "generator_attach_encoder: current device %d is not the generator's (%d)",
               dev, gen->device);
    hipStream_t st = (hipStream_t)stream;
    enc_free(gen);                                   // (a second call replaces the first)
    NbGenerator::Encoder& E = gen->enc;
    std::vector<void*> temps;
    bool ok = true;
    auto alloc = [&](size_t bytes, std::vector<void*>& list) -> void* {
        void* p = nullptr;
        if (!ok || bytes == 0) return nullptr;
        if (hipMalloc(&p, (bytes + 255) / 256 * 256) != hipSuccess) {
            ok = false;
            nb_set_error("generator_attach_encoder: hipMalloc of %zu bytes failed", bytes);
            return nullptr;
        }
        list.push_back(p);
        return p;
    };
    auto finish = [&](int code) {
        (void)hipStreamSynchronize(st);
        for (void* p : temps) (void)hipFree(p);
        if (code != NB_OK) enc_free(gen);
        return code;
    };
    const bool f8 = gen->opts.conv_mode == NB_CONV_F8;
    const float* const* P = (const float* const*)enc_params_dev;
    for (int l = 0; l < 7; ++l) {
        const EncLayer& L = kEncLayers[l];
        const float* const* p = P + l * kEncParamsPerLayer;       // weight, bias, gamma, beta, mean, var
        const int per = L.c_in * L.k * L.k, ld = l == 0 ? 50 : per;
        float* w = (float*)alloc((size_t)L.c_out * ld * sizeof(float), l == 0 ? E.allocs : temps);
        float* b = (float*)alloc((size_t)L.c_out * sizeof(float), E.allocs);
        if (!ok) return finish(NB_ELAUNCH);
        hipLaunchKernelGGL(enc_fold_bn_kernel, dim3(nb_cdiv(L.c_out * ld, 256)), dim3(256), 0, st, p[0], p[1], p[2], p[3], p[4], p[5], L.c_out,
                           per, ld, w, b);
        if (hipGetLastError() != hipSuccess) {
            nb_set_error("generator_attach_encoder: launch of the BatchNorm fold failed");
            return finish(NB_ELAUNCH);
        }
        if (l == 0) {
            E.w50 = w;
            E.b0 = b;
            continue;
        }
        // encoder.pack_enc_weight_h3 / pack_enc_weight_f8: the containers with c_out padded to 128
        const size_t bytes = (size_t)(L.c_in + 15) / 16 * 9 * 4 * ((L.c_out + 127) / 128 * 128) * 8 * sizeof(_Float16);
        E.b[l - 1] = b;
        E.w_h3[l - 1] = alloc(bytes, E.allocs);
        if (f8) E.w_f8[l - 1] = alloc(bytes, E.allocs);
        if (!ok) return finish(NB_ELAUNCH);
        int rc = nb_pack_conv_weight_h3_dev(w, L.c_out, L.c_in, 128, 0, E.w_h3[l - 1], st);
        if (!rc && f8) rc = pack_h3f8(w, L.c_out, L.c_in, 128, E.w_f8[l - 1], st);
        if (rc) return finish(rc);
    }
    // workspaces: the largest each gets at any batch up to n_max (below batch 8, and always for h3 / f32 generators, the stem writes the
    // 64-channel full-resolution tensor that the fused f8 launch never creates)
    size_t need_ping = 0;
    for (int n = 1; n <= gen->n_max; ++n) enc_walk(gen, nullptr, n, st, nullptr, false, &need_ping, nullptr, nullptr);
    const int R = gen->cfg.R;
    E.ping[0] = alloc(need_ping, E.allocs);
    E.ping[1] = alloc(need_ping, E.allocs);
    E.feat0 = (float*)alloc((size_t)gen->n_max * 16 * (R / 8) * (R / 8) * sizeof(float), E.allocs);
    E.up = alloc(h2_bytes(gen->n_max, 16, (R / 4) * (R / 4)), E.allocs);
    if (!ok) return finish(NB_ELAUNCH);
    if (hipStreamSynchronize(st) != hipSuccess) {
        nb_set_error("generator_attach_encoder: %s", hipGetErrorString(hipGetLastError()));
        return finish(NB_ELAUNCH);
    }
    E.preproc = preproc;
    return finish(NB_OK);
}

extern "C" int nb_generator_forward_geom(NbGenerator* gen, const NbGeneratorInputs* in, const float* geom, const NbGeneratorOutputs* out,
                                         int n, void* stream) {
    NB_REQUIRE(gen && in && out, "generator_forward_geom: null pointer");
    NB_REQUIRE(gen->enc.preproc >= 0, "generator_forward_geom: no encoder attached (nb_generator_attach_encoder)");
    for (int k = 0; k < 4; ++k)
        NB_REQUIRE(!in->geom[k], "generator_forward_geom: geometry feature %d given: the encoder computes them (pass stroke patches only)", k);
    NB_REQUIRE(geom, "generator_forward_geom: null stroke patches");
    if (const int rc = check_forward(gen, in, n, stream, "generator_forward_geom")) return rc;
    if (const int rc = check_modes_and_device(gen, in, stream, "generator_forward_geom")) return rc;
    NbGeneratorInputs io = *in;                      // the encoder fills io.geom[] before the walk reads them
    hipStream_t st = (hipStream_t)stream;
    const GeomHook hook = [&](const NbPassPlan& plan, unsigned* handed) {
        return enc_walk(gen, geom, n, st, &plan, true, nullptr, &io, handed);
    };
    WalkSink sink;
    sink.launch = true;
    return gen_walk(gen, &io, out, n, st, sink, &hook);
}

// ------------------------------------------------------------------------------------------------
// staged passes: the two halves of the painting engine's split around the feature-canvas blend (painting.PaintingHelper._schedule:
// SynthesisNetwork with _stop_after / _resume; the reference blends inside its one pass, networks_modified.py:168-222)
// ------------------------------------------------------------------------------------------------
namespace {

// the rules of a stage that need no handle (`who` prefixes the messages)
int check_stage(const NbGeneratorStage* stage, const char* who) {
    NB_REQUIRE(stage, "%s: null stage", who);
    NB_REQUIRE((stage->stop_res != 0) != (stage->resume_res != 0), "%s: exactly one of stop_res / resume_res must be set (got %d / %d)", who,
               stage->stop_res, stage->resume_res);
    const int res = stage->stop_res ? stage->stop_res : stage->resume_res;
    NB_REQUIRE(res >= 4 && (res & (res - 1)) == 0, "%s: %d is not a block resolution (a power of two in [4, R])", who, res);
    return NB_OK;
}

}  // namespace

extern "C" int nb_generator_forward_staged(NbGenerator* gen, const NbGeneratorInputs* in, const float* geom, const NbGeneratorStage* stage,
                                           const NbGeneratorOutputs* out, int n, void* stream) {
    const char* who = "generator_forward_staged";
    if (const int rc = check_stage(stage, who)) return rc;
    NB_REQUIRE(gen && in, "%s: null pointer", who);
    const GenCfg& cfg = gen->cfg;
    const int res = stage->stop_res ? stage->stop_res : stage->resume_res;
    NB_REQUIRE(res <= cfg.R, "%s: %d is not a block resolution (a power of two in [4, %d])", who, res, cfg.R);
    const int ng = (int)cfg.geom_res.size();
    bool need_geom = false;                          // does the pass read a geometry feature at all?
    if (stage->stop_res) {
        NB_REQUIRE(stage->features_out, "%s: null features_out", who);
        NB_REQUIRE(!out || !(out->rgba_u8 || out->rgba || out->img || out->uvs || out->colors),
                   "%s: a pass that stops after a block has no ToRGB: every output pointer must be NULL", who);
        need_geom = ng > 0;
    } else {
        NB_REQUIRE(stage->features_in, "%s: null features_in", who);
        NB_REQUIRE(out, "%s: null outputs", who);
        for (int k = 0; k < ng; ++k) need_geom = need_geom || cfg.geom_res[k] >= res;
    }
    if (const int rc = check_forward(gen, in, n, stream, who)) return rc;
    const bool encode = need_geom && geom != nullptr;
    if (encode) {
        NB_REQUIRE(gen->enc.preproc >= 0, "%s: stroke patches given but no encoder attached (nb_generator_attach_encoder)", who);
        for (int k = 0; k < 4; ++k)
            NB_REQUIRE(!in->geom[k], "%s: geometry feature %d given: the encoder computes them (pass stroke patches only)", who, k);
    } else if (need_geom) {
        for (int k = 0; k < ng; ++k)
            NB_REQUIRE(in->geom[k] || (stage->resume_res && cfg.geom_res[k] < res), "%s: geometry feature %d is NULL", who, k);
    }
    if (const int rc = check_modes_and_device(gen, in, stream, who)) return rc;
    NbGeneratorInputs io = *in;
    if (!need_geom)
        for (int k = 0; k < 4; ++k) io.geom[k] = nullptr;
    hipStream_t st = (hipStream_t)stream;
    const GeomHook hook = [&](const NbPassPlan& plan, unsigned* handed) {
        return enc_walk(gen, geom, n, st, &plan, true, nullptr, &io, handed);
    };
    WalkSink sink;
    sink.launch = true;
    return gen_walk(gen, &io, out, n, st, sink, encode ? &hook : nullptr, stage);
}

extern "C" int nb_generator_describe_staged(NbGenerator* gen, int n, int stop_res, int resume_res, char* buf, int len) {
    const char* who = "generator_describe_staged";
    NbGeneratorStage sg{};
    sg.stop_res = stop_res;
    sg.resume_res = resume_res;
    if (const int rc = check_stage(&sg, who)) return rc;
    NB_REQUIRE(gen && buf && len > 0, "%s: bad arguments", who);
    const int res = stop_res ? stop_res : resume_res, R = gen->cfg.R;
    NB_REQUIRE(res <= R, "%s: %d is not a block resolution (a power of two in [4, %d])", who, res, R);
    NB_REQUIRE(n >= 1 && n <= gen->n_max, "%s: batch %d outside [1, n_max = %d]", who, n, gen->n_max);
    NbPassPlan plan;
    if (const int rc = gen->plan(n, true, &plan, stop_res, resume_res)) return rc;
    std::string s;
    for (int i = 0; i < plan.num_layers; ++i) {
        const int br = gen->cfg.layers[i].block_res;
        if (stop_res ? br <= stop_res : br > resume_res) s += gen->cfg.layers[i].name + "=" + plan.layers[i].kernel + "\n";
    }
    if (resume_res) {                                // the tail's ToRGB: fused into the last conv, or on its own (always behind block R)
        const NbLayerPlan& last = plan.layers[plan.num_layers - 1];
        s += fmt("synthesis.b%d.torgb=", R) + (resume_res < R && last.fused_torgb ? last.kernel : "torgb_triad_kernel") + "\n";
    }
    NB_REQUIRE(len > (int)s.size(), "%s: buffer of %d bytes, %d needed", who, len, (int)s.size() + 1);
    memcpy(buf, s.c_str(), s.size() + 1);
    return NB_OK;
}

// ------------------------------------------------------------------------------------------------
// brush noise sets: a projected brush's noise_const replacements and their transposes at fixed addresses (include/neube_hip.h)
// ------------------------------------------------------------------------------------------------
namespace {

void brush_noise_free(NbBrushNoise* bn, int device) {
    int prev = 0;
    const bool have = hipGetDevice(&prev) == hipSuccess;
    if ((bn->buf || bn->tables) && hipSetDevice(device) == hipSuccess) {
        (void)hipDeviceSynchronize();
        if (bn->buf) (void)hipFree(bn->buf);
        if (bn->tables) (void)hipFree(bn->tables);
    }
    if (have) (void)hipSetDevice(prev);
    delete bn;
}

// one nb_brush_noise_build_f32 launch into the set; a NULL a[i] / b[i] is the checkpoint's buffer, b == NULL a plain copy
int brush_noise_fill(NbBrushNoise* bn, const float* const* a, const float* const* b, float wa, float wb, void* stream) {
    const NbGenerator* g = bn->gen;
    const int nL = (int)g->L.size();
    NbBrushNoiseLayer layers[NB_PLAN_MAX_LAYERS];
    for (int i = 0; i < nL; ++i) {
        const float* ck = g->L[i].noise_const;
        layers[i] = NbBrushNoiseLayer{a && a[i] ? a[i] : ck, b ? (b[i] ? b[i] : ck) : nullptr, bn->nc[i], bn->nc_t[i],
                                      g->cfg.layers[i].block_res, 0};
    }
    return nb_brush_noise_build_f32(layers, nL, wa, wb, stream);
}

}  // namespace

extern "C" int nb_brush_noise_create(NbGenerator* gen, void* stream, NbBrushNoise** out) {
    NB_REQUIRE(out, "brush_noise_create: null output handle");
    *out = nullptr;
    NB_REQUIRE(gen, "brush_noise_create: null generator");
    int dev = -1;
    NB_REQUIRE(hipGetDevice(&dev) == hipSuccess && dev == gen->device, "brush_noise_create: current device %d is not the generator's (%d)", dev,
               gen->device);
    const int nL = (int)gen->L.size();
    size_t floats = 0;
    // (every image on a 256-byte boundary, as the checkpoint's own copies are)
    auto padded = [](const GenLayer& s) { return ((size_t)s.block_res * s.block_res + 63) / 64 * 64; };
    for (const GenLayer& s : gen->cfg.layers) floats += 2 * padded(s);
    NbBrushNoise* bn = new NbBrushNoise();
    bn->gen = gen;
    const size_t table_bytes = gen->host_tables.size() * sizeof(NbLayerDesc);
    if (hipMalloc((void**)&bn->buf, floats * sizeof(float)) != hipSuccess || hipMalloc((void**)&bn->tables, table_bytes) != hipSuccess) {
        nb_set_error("brush_noise_create: hipMalloc of %zu bytes failed", floats * sizeof(float) + table_bytes);
        brush_noise_free(bn, gen->device);
        return NB_ELAUNCH;
    }
    float* p = bn->buf;
    for (const GenLayer& s : gen->cfg.layers) {
        bn->nc.push_back(p);
        bn->nc_t.push_back(p + padded(s));
        p += 2 * padded(s);
    }
    // the handle's tables with noise_const pointing into the set (where a table has it cleared it stays cleared)
    std::vector<NbLayerDesc> descs = gen->host_tables;
    for (int first = 0; first <= nL; ++first)
        for (int i = 0; i < nL; ++i) {
            NbLayerDesc& d = descs[(size_t)first * (nL + 1) + i];
            if (d.noise_const) d.noise_const = bn->nc[i];
        }
    int rc = brush_noise_fill(bn, nullptr, nullptr, 1.f, 0.f, stream);
    if (rc == NB_OK && (hipMemcpyAsync(bn->tables, descs.data(), table_bytes, hipMemcpyHostToDevice, (hipStream_t)stream) != hipSuccess ||
                        hipStreamSynchronize((hipStream_t)stream) != hipSuccess)) {
        nb_set_error("brush_noise_create: %s", hipGetErrorString(hipGetLastError()));
        rc = NB_ELAUNCH;
    }
    if (rc != NB_OK) {
        brush_noise_free(bn, gen->device);
        return rc;
    }
    gen->sets.push_back(bn);
    *out = bn;
    return NB_OK;
}

extern "C" int nb_brush_noise_load(NbBrushNoise* bn, const float* const* a_dev, const float* const* b_dev, float alpha, void* stream) {
    NB_REQUIRE(bn, "brush_noise_load: null set");
    NB_REQUIRE(bn->gen, "brush_noise_load: the set's generator has been destroyed");
    NB_REQUIRE(a_dev, "brush_noise_load: null buffer array (a NULL entry stands for the checkpoint's buffer, the array itself may not be NULL)");
    int dev = -1;
    NB_REQUIRE(hipGetDevice(&dev) == hipSuccess && dev == bn->gen->device, "brush_noise_load: current device %d is not the generator's (%d)",
               dev, bn->gen->device);
    return brush_noise_fill(bn, a_dev, b_dev, alpha, (float)(1.0 - (double)alpha), stream);
}

extern "C" int nb_generator_bind_brush_noise(NbGenerator* gen, NbBrushNoise* bn) {
    NB_REQUIRE(gen, "generator_bind_brush_noise: null generator");
    NB_REQUIRE(!bn || bn->gen == gen, "generator_bind_brush_noise: the set belongs to another generator");
    gen->brush = bn;
    return NB_OK;
}

extern "C" int nb_brush_noise_destroy(NbBrushNoise* bn) {
    if (!bn) return NB_OK;
    int device = 0;
    if (NbGenerator* g = bn->gen) {
        device = g->device;
        if (g->brush == bn) g->brush = nullptr;
        for (size_t k = 0; k < g->sets.size(); ++k)
            if (g->sets[k] == bn) {
                g->sets.erase(g->sets.begin() + k);
                break;
            }
    } else {
        (void)hipGetDevice(&device);              // (an orphan: its generator went first, on the device that was current then)
    }
    brush_noise_free(bn, device);
    return NB_OK;
}
