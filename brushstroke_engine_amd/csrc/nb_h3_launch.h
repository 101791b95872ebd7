// Host-side launcher set-up shared by the split-f16 convolution families (nb_modconv_up1_h3.hip, nb_modconv_up2_h3.hip,
// nb_modconv_up2v.hip): the zero page, the timestamp buffer, the CU count, the noise source, the common argument checks.
#pragma once
#include "nb_h3_common.h"

extern "C" const float* nb_zero_page_ptr(void);     // nb_modconv.hip

// debug: per-workgroup phase timestamps of the next h3 launches (nb_debug_set_timestamps, nb_modconv_up1_h3.hip)
extern unsigned long long* g_tstamps;
extern int g_tstamps_cap;
// workgroups per CU of the persistent launches (NB_PERSIST_WGS_PER_CU, nb_modconv_up1_h3.hip)
extern int g_persist_wgs_per_cu;

// compute units of the current device, asked once (256 = MI355X if the runtime will not say)
inline int nb_num_cus() {
    static int ncu = 0;
    if (!ncu) {
        int dev = 0, v = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) v = 256;
        ncu = v;
    }
    return ncu;
}

// `noise` / `noise_stride_n` of the entry points -> kernel fields: a [n or 1][H][W] tensor, or (NB_NOISE_IN_KERNEL) a host
// NbNoiseSrc describing how the kernel computes the noise itself
static int nb_noise_src_setup(const float* noise, int64_t stride_n, int ho, int wo, const float** k_noise, long long* k_stride, NbNoiseSrcDev* k_src) {
    *k_src = NbNoiseSrcDev{nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0};
    if (stride_n != NB_NOISE_IN_KERNEL) { *k_noise = noise; *k_stride = stride_n; return NB_OK; }
    const NbNoiseSrc* s = reinterpret_cast<const NbNoiseSrc*>(noise);
    if (!s || !s->noise_const_t || !s->noise_lin || !s->noise_strength || ((s->norm_pos != nullptr) == (s->positions != nullptr))) return NB_EINVAL;
    if (s->res != ho || s->res != wo || (s->positions && s->img_resolution < 2)) return NB_EINVAL;
    *k_src = NbNoiseSrcDev{s->noise_const_t, s->noise_lin, s->noise_strength, s->norm_pos, (const long long*)s->positions, s->res, s->img_resolution};
    *k_noise = nullptr; *k_stride = 0;
    return NB_OK;
}

// One conv call's arguments, as the entry points of both families take them (h x w = the INPUT image)
struct H3ConvArgs {
    const void* x_h2; int c_in; const void* w_h3; const float* dcoefs; const float* noise; int64_t noise_stride_n; const float* bias;
    float* y; void* y_h2; const float* next_styles; int next_stride, c_next, n, h, w, c_out;
    float alpha, gain, clamp;
    int out_fmt;
};

// What nb_up1_h3_impl and nb_up2_h3_impl share, from the hand-off check on (the operand-format and pointer checks in front of it differ
// per family): checks, zero page, noise source (output = up * h x up * w), every field of P (H3Params / H3Up2Params) that does not
// depend on the tile.
// `name` = the entry's message prefix; `shape_ok` / `shape_rule` = the family's image-size rule.  The two families have always
// reported a bad slope and a bad shape in opposite orders (`slope_first`: up=1); callers may rely on which message they get.
template <class P>
static int nb_h3_launch_setup(P& p, const char* name, const H3ConvArgs& a, int up, bool shape_ok, const char* shape_rule, bool slope_first) {
    NB_REQUIRE(!a.y_h2 || (a.next_styles && a.c_out % 8 == 0 && a.c_next >= a.c_out && a.next_stride >= a.c_out && (uintptr_t)a.y_h2 % 16 == 0),
               "%s: H2 output needs the consumer's styles, c_out %% 8 == 0 and c_next >= c_out", name);
    NB_REQUIRE(a.n > 0 && a.n <= 65535 && a.c_in > 0 && a.c_out > 0, "%s: bad sizes", name);
    if (slope_first || shape_ok)
        NB_REQUIRE(a.alpha >= 0.f && a.alpha <= 1.f && a.gain > 0.f, "%s: leaky-ReLU slope must lie in [0, 1] and the gain be positive (got %g, %g)", name, a.alpha, a.gain);
    NB_REQUIRE(shape_ok, "%s: needs %s (got %dx%d)", name, shape_rule, a.h, a.w);
    NB_REQUIRE(((uintptr_t)a.x_h2 | (uintptr_t)a.w_h3 | (uintptr_t)a.y) % 16 == 0, "%s: pointers must be 16-byte aligned", name);
    p.x = (const _Float16*)a.x_h2; p.wts = (const _Float16*)a.w_h3; p.dcoefs = a.dcoefs; p.noise = a.noise; p.bias = a.bias; p.y = a.y;
    p.zeros = nb_zero_page_ptr();
    NB_REQUIRE(p.zeros, "%s: could not allocate the zero page", name);
    p.noise_stride_n = a.noise_stride_n;
    NB_REQUIRE(nb_noise_src_setup(a.noise, a.noise_stride_n, up * a.h, up * a.w, &p.noise, &p.noise_stride_n, &p.nsrc) == NB_OK, "%s: bad NbNoiseSrc (needs the "
               "transposed constant, the grid row, the strength, exactly one of norm_pos / positions, and res = the %dx%d output)", name, up * a.h, up * a.w);
    p.c8 = (a.c_in + 7) / 8; p.nchunks = (a.c_in + 15) / 16; p.c_out = a.c_out; p.co_ld = (a.c_out + 63) / 64 * 64; p.h = a.h; p.w = a.w;
    p.dbg = g_nb_debug_flags; p.stagger_ticks = g_nb_stagger_ticks;            // (developer hooks: nb_debug_set_flags / nb_debug_set_stagger)
    p.alpha = a.alpha; p.gain = a.gain; p.clamp = a.clamp;
    p.yh2 = (_Float16*)a.y_h2; p.next_styles = a.next_styles; p.next_stride = a.next_stride; p.c8_next = (a.c_next + 7) / 8;
    p.out_f8 = a.out_fmt;
    return NB_OK;
}
