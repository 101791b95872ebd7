// The whole generator behind one C handle (include/neube_hip.h, "the whole generator"): the handle, and the host orchestration of one
// forward pass -- the launches and per-batch kernel choices of SynthesisNetwork._run_layers (networks.py) on one stream, without torch.
// Its weight packers live in nb_weight_pack.hip, its tables and planner in nb_gen_plan.hip, the geometry encoder behind the handle in
// nb_gen_encoder.hip, brush noise sets in nb_brush_noise.hip; nb_gen_internal.h holds what they share.
//
// The orchestration is a single walk (gen_walk) used two ways: to size the workspaces at creation (every batch up to n_max, whole
// passes and every stage) and to enqueue a forward pass -- whole, or one stage of the painting engine's split (NbGeneratorStage: a
// head that stops after a block, a tail that resumes behind it).  It differs from SynthesisNetwork only in that the early geometry
// pack runs in-line on the one stream instead of on a side stream (same kernel, same inputs: same bits).
#include "nb_gen_internal.h"

// ------------------------------------------------------------------------------------------------
// small kernels of the generator object
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

namespace nbgen __attribute__((visibility("hidden"))) {

int require_current_device(const NbGenerator* gen, const char* who) {
    int dev = -1;
    NB_REQUIRE(hipGetDevice(&dev) == hipSuccess && dev == gen->device, "%s: current device %d is not the generator's (%d)", who, dev,
               gen->device);
    return NB_OK;
}

PartPack part_pack(const NbGenerator* g, int consumer, int gch) {
    const GenLayer& sc = g->cfg.layers[consumer];
    const int c_prod = sc.in_ch - gch;
    return PartPack{c_prod, g->L[consumer].styles + c_prod, sc.in_ch, (sc.in_ch + 7) / 8, c_prod / 8};
}

namespace {

// One forward pass in the steps of SynthesisNetwork._prepare + _run_layers (gen_walk calls them in order): what the pass is given,
// what is fixed once it is planned, and what moves from step to step (as _Pass in networks.py).
struct Walk {
    NbGenerator* const g;
    const NbGeneratorInputs* const in;
    const NbGeneratorOutputs* const out;
    const int n;
    const hipStream_t st;
    const WalkSink sink;
    const NbGeneratorStage* const stage;
    const GenCfg& cfg = g->cfg;
    const std::vector<GenLayer>& specs = cfg.layers;
    const int nL = (int)specs.size(), R = cfg.R, c_last = cfg.channels(R);
    const float clamp = cfg.c.conv_clamp < 0.f ? -1.f : cfg.c.conv_clamp;
    const bool cnoise = in->noise_mode == NB_NOISE_CONST, snoise = in->noise_mode == NB_NOISE_SEEDED;
    const int64_t* const ipos = cnoise ? in->positions : nullptr;
    const NbBrushNoise* const bn = cnoise ? g->brush : nullptr;      // (the other noise modes ignore a bound set)
    const int stop_res = stage ? stage->stop_res : 0, resume_res = stage ? stage->resume_res : 0;
    float* const uvs = out->uvs ? out->uvs : g->uvs_ws;
    float* const img = out->img ? out->img : g->img_ws;
    float* const colors = out->colors ? out->colors : g->colors_ws;
    NbPassPlan plan{};
    const float* ws = in->ws;
    const float* npos_k = nullptr;                    // the batch's normalised positions, where one launch computes them
    const float* x = resume_res ? nullptr : g->const_rep;       // fp32 NCHW input of the next layer (NULL: handed over in operand format)
    int xc = cfg.channels(4);
    const float* x2 = nullptr;                        // geometry feature still to be concatenated
    int x2c = 0;
    void* xh2 = nullptr;                              // the next layer's complete operand-format input, when its producer wrote it
    int geo_idx = 0;

    bool head_last(int i) const { return stop_res && specs[i].up == 1 && specs[i].block_res == stop_res; }   // the tapped layer
    bool fused_torgb(int i) const { return plan.layers[i].fused_torgb && !head_last(i); }

    // ---- mapping (MappingNetwork.forward) ----
    int mapping() {
        if (ws) return NB_OK;
        const int w_dim = cfg.c.w_dim;
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
        return NB_OK;
    }

    // ---- noise sources (_prepare_noise_sources) ----
    int noise_sources() {
        if (plan.positions_once) {
            GEN_TRY(nb_norm_positions_f32(ipos, R, g->npos, n, st));
            npos_k = g->npos;
        }
        return NB_OK;
    }

    // ---- styles and noise images (_launch_styles_and_noise) ----
    int styles_and_noise() {
        const int n_tab = nL + 1, w_dim = cfg.c.w_dim;
        const int inkernel_from = plan.inkernel_from;      // first layer from which every layer computes its noise itself
        if (plan.styles_noise) {
            GEN_TRY(nb_styles_noise_f32(g->table(inkernel_from < 0 ? nL : inkernel_from, bn), n_tab, ws, cfg.num_ws, w_dim, nullptr, ipos, R, n, st));
            return NB_OK;
        }
        GEN_TRY((plan.styles_fast ? nb_styles_fast_f32 : nb_styles_f32)(g->table(nL), n_tab, ws, cfg.num_ws, w_dim, n, st));
        if (!(cnoise || snoise)) return NB_OK;
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
                GEN_TRY(nb_noise_seeded_f32(g->table(nL) + lo, lo, hi - lo, max_res, in->noise_seed, in->noise_offset, in->noise_state, n, st));
            else
                GEN_TRY(nb_noise_f32(g->table(nL, bn) + lo, hi - lo, max_res, npos_k, npos_k ? nullptr : ipos, R, n, st));
        }
        return NB_OK;
    }

    // ---- early geometry packs (_pack_geometry_early; in-line on the one stream) ----
    int early_geom_packs(unsigned handed) {
        for (int gi = 0; gi < (int)cfg.geom_res.size(); ++gi) {
            const NbGeomPlan& gp = plan.geom[gi];
            if (!gp.early_pack || ((handed >> gi) & 1)) continue;
            const int gres = cfg.geom_res[gi], gch = cfg.geom_ch[gi];
            const PartPack pp = part_pack(g, gp.consumer, gch);
            if (sink.sizing) g->need_pre[gi] = std::max(g->need_pre[gi], h2_bytes(n, pp.c_in, gres * gres));
            GEN_TRY(part_pack_fn(gp.fmt)(in->geom[gi], gch, pp.styles, pp.c_in, g->pre_h2[gi], pp.groups, pp.cg0, n, gres * gres, st));
        }
        return NB_OK;
    }

    // a block the resumed pass skips (_run_layers): its output is the caller's, and the geometry index moves on
    bool skipped(int i) {
        const GenLayer& s = specs[i];
        const int res = s.block_res;
        if (!(resume_res && res <= resume_res)) return false;
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
        return true;
    }

    int torgb(const float* features) {               // the ToRGB as a launch of its own
        GEN_TRY(nb_torgb_triad_f32(features, g->trgb_styles, c_last + 9, g->trgb_w, g->trgb_b, g->trgb_cb, clamp, nullptr, uvs, img, colors,
                                   in->user_colors, in->sfactor, in->render_mode, out->rgba, out->rgba_u8, n, c_last, R * R, st));
        return NB_OK;
    }

    // ---- one layer (_run_layer) ----
    int layer(int i) {
        const GenLayer& s = specs[i];
        const GenLayerDev& d = g->L[i];
        const NbLayerPlan& lp = plan.layers[i];
        const int res = s.block_res, ir = s.in_res();
        const float alpha = 0.2f, gain = g->act_gain;
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
            nstride = (cnoise && ipos == nullptr) ? 0 : (int64_t)res * res;      // (no positions: one image shared by the batch)
        }
        const bool to_caller = head_last(i);          // fp32 into the caller's buffer
        const bool fused = fused_torgb(i);
        const int gi_after = s.up == 1 ? cfg.geom_index(res) : -1;
        auto fp32_out = [&]() -> float* {              // the caller's buffer for the tapped layer, else the activation buffer x is not in
            if (to_caller) return stage->features_out;
            if (sink.sizing) g->need_act = std::max(g->need_act, (size_t)n * s.out_ch * res * res * sizeof(float));
            return x == g->act[0] ? g->act[1] : g->act[0];
        };
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
            if (fused) {
                targs = NbTorgbArgs{g->trgb_styles, g->trgb_w, g->trgb_b, g->trgb_cb, nullptr, uvs, img, colors, in->user_colors,
                                    in->sfactor, out->rgba, out->rgba_u8, s.out_ch + 9, in->render_mode, clamp};
            } else if (lp.handoff) {
                if (gi_after >= 0 && plan.geom[gi_after].early_pack) {
                    next_h2 = g->pre_h2[gi_after];
                } else {
                    next_h2 = xh2 == g->h2[0] ? g->h2[1] : g->h2[0];
                    if (sink.sizing) g->need_h2 = std::max(g->need_h2, h2_bytes(n, specs[i + 1].in_ch, res * res));
                }
            } else {
                y = fp32_out();
            }
            const float* nst = next_h2 ? g->L[i + 1].styles : nullptr;
            const int c_next = next_h2 ? specs[i + 1].in_ch : 0;
            if (s.up == 1) {
                GEN_TRY(nb_modconv3x3_up1_h3_ex(xh2, s.in_ch, wts, d.dcoefs, noise, nstride, d.bias, y, next_h2, nst, c_next, c_next,
                                                fused ? &targs : nullptr, lp.kernel_fmt, lp.out_fmt, n, ir, ir, s.out_ch, alpha, gain, clamp,
                                                st));
            } else {
                GEN_TRY(nb_modconv3x3_up2_h3_ex(xh2, s.in_ch, wts, d.dcoefs, noise, nstride, d.bias, y, next_h2, nst, c_next, c_next,
                                                lp.kernel_fmt, lp.out_fmt, n, ir, ir, s.out_ch, alpha, gain, clamp, st));
            }
        } else {
            y = fp32_out();
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
        return NB_OK;
    }

    // ---- what follows a block's last layer (_finish_block): its ToRGB, the geometry feature of its resolution ----
    int finish_block(int i) {
        const int res = specs[i].block_res;
        if (res == R && !fused_torgb(i))
            if (const int rc = torgb(x)) return rc;
        if (cfg.geom_index(res) < 0) return NB_OK;
        const float* gf = in->geom[geo_idx];
        const int gch = cfg.geom_ch[geo_idx];
        if (xh2 && plan.geom[geo_idx].early_pack && xh2 == g->pre_h2[geo_idx]) {
            // packed at the start of the pass
        } else if (xh2) {
            // the block's last layer wrote its channels into the consumer's operands: the geometry channels go behind them
            const PartPack pp = part_pack(g, i + 1, gch);
            GEN_TRY(part_pack_fn(plan.layers[i + 1].in_fmt)(gf, gch, pp.styles, pp.c_in, xh2, pp.groups, pp.cg0, n, res * res, st));
        } else {
            x2 = gf;
            x2c = gch;
        }
        ++geo_idx;
        return NB_OK;
    }
};

void gen_free(NbGenerator* g) {
    if (!g) return;
    for (NbBrushNoise* s : g->sets) s->gen = nullptr;
    if (!g->mem.list.empty() || !g->enc.mem.list.empty()) {
        const DeviceScope scope(g->device);
        if (scope.ok) {
            (void)hipDeviceSynchronize();
            g->mem.free_all();
            g->enc.mem.free_all();
        }
    }
    delete g;
}

// the rules of a stage that need no handle (`who` prefixes the messages)
int check_stage(int stop_res, int resume_res, const char* who) {
    NB_REQUIRE((stop_res != 0) != (resume_res != 0), "%s: exactly one of stop_res / resume_res must be set (got %d / %d)", who, stop_res,
               resume_res);
    const int res = stop_res ? stop_res : resume_res;
    NB_REQUIRE(res >= 4 && (res & (res - 1)) == 0, "%s: %d is not a block resolution (a power of two in [4, R])", who, res);
    return NB_OK;
}

// The kernels of a pass at batch n, one "layer=kernel" line each: a whole pass (stop_res = resume_res = 0) or one stage.  The
// arguments are the caller's to check, but for the batch.
int describe(NbGenerator* gen, int n, int stop_res, int resume_res, char* buf, int len, const char* who) {
    NB_REQUIRE(n >= 1 && n <= gen->n_max, "%s: batch %d outside [1, n_max = %d]", who, n, gen->n_max);
    NbPassPlan plan;
    if (const int rc = gen->plan(n, true, &plan, stop_res, resume_res)) return rc;
    const int R = gen->cfg.R;
    std::string s;
    for (int i = 0; i < plan.num_layers; ++i) {
        const int br = gen->cfg.layers[i].block_res;
        if (stop_res ? br <= stop_res : br > resume_res) s += gen->cfg.layers[i].name + "=" + plan.layers[i].kernel + "\n";
    }
    if (!stop_res) {                                 // the ToRGB: fused into the last conv, or on its own (always behind block R)
        const NbLayerPlan& last = plan.layers[plan.num_layers - 1];
        s += fmt("synthesis.b%d.torgb=", R) + (resume_res < R && last.fused_torgb ? last.kernel : "torgb_triad_kernel") + "\n";
    }
    NB_REQUIRE(len > (int)s.size(), "%s: buffer of %d bytes, %d needed", who, len, (int)s.size() + 1);
    memcpy(buf, s.c_str(), s.size() + 1);
    return NB_OK;
}

}  // namespace

// One forward pass: SynthesisNetwork._prepare + _run_layers for render_triad (constant, seeded or no noise, no feature taps / blending),
// following the pass's plan.  stage (validated by the caller) makes it one half of the painting engine's split: stop_res = the pass of
// `_stop_after` (ends with block stop_res, whose last layer writes stage->features_out; no ToRGB), resume_res = the pass of `_resume`
// (starts behind block resume_res from stage->features_in).
int gen_walk(NbGenerator* g, const NbGeneratorInputs* in, const NbGeneratorOutputs* out, int n, hipStream_t st, const WalkSink& sink,
             const GeomHook* geom_hook, const NbGeneratorStage* stage) {
    static const NbGeneratorOutputs no_outputs{};
    Walk w{g, in, out ? out : &no_outputs, n, st, sink, stage};
    int rc = g->plan(n, w.ipos != nullptr, &w.plan, w.stop_res, w.resume_res);
    if (!rc) rc = w.mapping();
    if (!rc) rc = w.noise_sources();
    if (!rc) rc = w.styles_and_noise();
    // ---- geometry from stroke patches (_encode_lazy_geometry) ----
    unsigned handed = 0;
    if (!rc && geom_hook && sink.launch) rc = (*geom_hook)(w.plan, &handed);
    if (!rc) rc = w.early_geom_packs(handed);
    // ---- the layers (_run_layers) ----
    for (int i = 0; i < w.nL && !rc; ++i) {
        if (w.skipped(i)) continue;
        rc = w.layer(i);
        if (w.head_last(i)) return rc;               // (_stop_after: no ToRGB, no geometry behind the block)
        if (!rc && w.specs[i].up == 1) rc = w.finish_block(i);
    }
    // resumed behind the last block: nothing but its ToRGB is left
    if (!rc && w.resume_res == w.R) rc = w.torgb(stage->features_in);
    return rc;
}

int check_forward(NbGenerator* gen, const NbGeneratorInputs* in, int n, const char* who) {
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
    if (const int rc = require_current_device(gen, who)) return rc;
    if (stream) {
        hipDevice_t sdev = -1;
        NB_REQUIRE(hipStreamGetDevice((hipStream_t)stream, &sdev) == hipSuccess && sdev == gen->device,
                   "%s: the stream belongs to device %d, the generator to %d", who, (int)sdev, gen->device);
    }
    return NB_OK;
}

int run_forward(NbGenerator* gen, const NbGeneratorInputs* in, const float* patches, const NbGeneratorStage* stage,
                const NbGeneratorOutputs* out, int n, void* stream) {
    NbGeneratorInputs io = *in;
    hipStream_t st = (hipStream_t)stream;
    WalkSink sink;
    sink.launch = true;
    const GeomHook hook = [&](const NbPassPlan& plan, unsigned* handed) {
        return enc_walk(gen, patches, n, st, &plan, sink, nullptr, &io, handed);
    };
    return gen_walk(gen, &io, out, n, st, sink, patches ? &hook : nullptr, stage);
}

}  // namespace nbgen

using namespace nbgen;

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
    DeviceAllocs& mem = g->mem;
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
        float* p = (float*)mem.get(bytes);
        if (!mem.ok) return fail(NB_ELAUNCH);
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
        float* mw = (float*)mem.get(wn * sizeof(float));
        float* mb = (float*)mem.get((size_t)C.c.mapping_layers * w_dim * sizeof(float));
        if (!mem.ok) return fail(NB_ELAUNCH);
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
    g->const_rep = (float*)mem.get((size_t)n_max * c4 * 16 * sizeof(float));
    if (!mem.ok) return fail(NB_ELAUNCH);
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
        d.wpk = (float*)mem.get((size_t)(s.in_ch + 7) / 8 * 8 * 9 * ((s.out_ch + 31) / 32 * 32) * sizeof(float));
        d.wsq = (float*)mem.get((size_t)s.in_ch * s.out_ch * sizeof(float));
        d.noise_lin = (float*)mem.get((size_t)r * sizeof(float));
        d.noise_const_t = (float*)mem.get((size_t)r * r * sizeof(float));
        d.styles = (float*)mem.get((size_t)n_max * s.in_ch * sizeof(float));
        d.dcoefs = (float*)mem.get((size_t)n_max * s.out_ch * sizeof(float));
        d.noise = (float*)mem.get((size_t)n_max * r * r * sizeof(float));
        const size_t h3_bytes = h3_weight_bytes(s.in_ch, s.out_ch, 64);
        if (packs & NB_PACK_H3) d.w_h3 = mem.get(h3_bytes);
        if (packs & NB_PACK_F8) d.w_f8 = mem.get(h3_bytes);
        if (packs & NB_PACK_H3_UP2) d.w_h3_up2 = mem.get(4 * h3_bytes);
        if (!mem.ok) return fail(NB_ELAUNCH);
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
    g->trgb_styles = (float*)mem.get((size_t)n_max * (c_last + 9) * sizeof(float));
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
    g->tables = (NbLayerDesc*)mem.get(descs.size() * sizeof(NbLayerDesc));
    g->ws_buf = (float*)mem.get((size_t)n_max * C.num_ws * w_dim * sizeof(float));
    g->npos = (float*)mem.get((size_t)n_max * 2 * sizeof(float));
    g->uvs_ws = (float*)mem.get((size_t)n_max * 3 * C.R * C.R * sizeof(float));
    g->img_ws = (float*)mem.get((size_t)n_max * 3 * C.R * C.R * sizeof(float));
    g->colors_ws = (float*)mem.get((size_t)n_max * 9 * sizeof(float));
    if (!mem.ok) return fail(NB_ELAUNCH);
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
        g->act[0] = (float*)mem.get(g->need_act); g->act[1] = (float*)mem.get(g->need_act);
        g->h2[0] = mem.get(g->need_h2); g->h2[1] = mem.get(g->need_h2);
        for (size_t k = 0; k < C.geom_res.size(); ++k) g->pre_h2[k] = mem.get(g->need_pre[k]);
        if (!mem.ok) return fail(NB_ELAUNCH);
    }
    if (hipStreamSynchronize(st) != hipSuccess) {
        nb_set_error("generator_create: %s", hipGetErrorString(hipGetLastError()));
        return fail(NB_ELAUNCH);
    }
    *out = g;
    return NB_OK;
}

extern "C" int nb_generator_forward(NbGenerator* gen, const NbGeneratorInputs* in, const NbGeneratorOutputs* out, int n, void* stream) {
    NB_REQUIRE(gen && in && out, "generator_forward: null pointer");
    if (const int rc = check_forward(gen, in, n, "generator_forward")) return rc;
    for (size_t k = 0; k < gen->cfg.geom_res.size(); ++k) NB_REQUIRE(in->geom[k], "generator_forward: geometry feature %d is NULL", (int)k);
    if (const int rc = check_modes_and_device(gen, in, stream, "generator_forward")) return rc;
    return run_forward(gen, in, nullptr, nullptr, out, n, stream);
}

extern "C" int nb_generator_describe(NbGenerator* gen, int n, char* buf, int len) {
    NB_REQUIRE(gen && buf && len > 0, "generator_describe: bad arguments");
    return describe(gen, n, 0, 0, buf, len, "generator_describe");
}

// staged passes: the two halves of the painting engine's split around the feature-canvas blend (painting.PaintingHelper._schedule:
// SynthesisNetwork with _stop_after / _resume; the reference blends inside its one pass, networks_modified.py:168-222)
extern "C" int nb_generator_forward_staged(NbGenerator* gen, const NbGeneratorInputs* in, const float* geom, const NbGeneratorStage* stage,
                                           const NbGeneratorOutputs* out, int n, void* stream) {
    const char* who = "generator_forward_staged";
    NB_REQUIRE(stage, "%s: null stage", who);
    if (const int rc = check_stage(stage->stop_res, stage->resume_res, who)) return rc;
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
    if (const int rc = check_forward(gen, in, n, who)) return rc;
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
    return run_forward(gen, &io, encode ? geom : nullptr, stage, out, n, stream);
}

extern "C" int nb_generator_describe_staged(NbGenerator* gen, int n, int stop_res, int resume_res, char* buf, int len) {
    const char* who = "generator_describe_staged";
    if (const int rc = check_stage(stop_res, resume_res, who)) return rc;
    NB_REQUIRE(gen && buf && len > 0, "%s: bad arguments", who);
    const int res = stop_res ? stop_res : resume_res, R = gen->cfg.R;
    NB_REQUIRE(res <= R, "%s: %d is not a block resolution (a power of two in [4, %d])", who, res, R);
    return describe(gen, n, stop_res, resume_res, buf, len, who);
}
