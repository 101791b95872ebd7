// The generator's configuration and planner (host only): the parameter and layer tables of a GeneratorConfig
// (config.GeneratorConfig, weights.random_state_dict) and the per-batch layer plan.  The per-batch kernel decisions of a pass live in
// one place, the planner (nb_synthesis_plan): SynthesisNetwork (networks.py) and the walk of nb_generator.hip both follow its plan.
#include "nb_gen_internal.h"

namespace nbgen __attribute__((visibility("hidden"))) {

std::string fmt(const char* f, int a) {
    char b[96];
    snprintf(b, sizeof(b), f, a);
    return b;
}

void add_param(std::vector<GenParam>& params, const std::string& name, std::initializer_list<int64_t> shape) {
    GenParam p;
    p.name = name;
    p.ndim = (int)shape.size();
    int k = 0;
    for (int64_t v : shape) p.shape[k++] = v;
    for (; k < 4; ++k) p.shape[k] = 0;
    params.push_back(p);
}

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
    std::vector<GenParam>& ps = g.params;
    for (int i = 0; i < c->mapping_layers; ++i) {
        add_param(ps, fmt("mapping.fc%d.weight", i), {c->w_dim, i == 0 ? c->z_dim : c->w_dim});
        add_param(ps, fmt("mapping.fc%d.bias", i), {c->w_dim});
    }
    add_param(ps, "mapping.w_avg", {c->w_dim});
    add_param(ps, "synthesis.b4.const", {g.channels(4), 4, 4});
    for (int res : g.blocks) add_param(ps, fmt("synthesis.b%d.resample_filter", res), {4, 4});
    for (const GenLayer& l : g.layers) {
        add_param(ps, l.name + ".weight", {l.out_ch, l.in_ch, 3, 3});
        add_param(ps, l.name + ".noise_strength", {});
        add_param(ps, l.name + ".bias", {l.out_ch});
        add_param(ps, l.name + ".noise_grid", {1, l.block_res, l.block_res, 2});
        add_param(ps, l.name + ".resample_filter", {4, 4});
        add_param(ps, l.name + ".noise_const", {l.block_res, l.block_res});
        add_param(ps, l.name + ".affine.weight", {l.in_ch, c->w_dim});
        add_param(ps, l.name + ".affine.bias", {l.in_ch});
    }
    const std::string t = fmt("synthesis.b%d.torgb", R);
    const int cl = g.channels(R);
    add_param(ps, t + ".weight", {3, cl, 1, 1});
    add_param(ps, t + ".bias", {3});
    add_param(ps, t + ".color_bias", {9});
    add_param(ps, t + ".affine.weight", {cl + 9, c->w_dim});
    add_param(ps, t + ".affine.bias", {cl + 9});
    return NB_OK;
}

static int copy_name(const std::string& s, char* buf, int len) {
    if (!buf) return NB_OK;
    NB_REQUIRE(len > (int)s.size(), "generator: name buffer too short (%d bytes for \"%s\")", len, s.c_str());
    memcpy(buf, s.c_str(), s.size() + 1);
    return NB_OK;
}

int param_info(const GenParam& p, char* name, int len, int64_t shape[4], int* ndim) {
    if (shape) for (int k = 0; k < 4; ++k) shape[k] = p.shape[k];
    if (ndim) *ndim = p.ndim;
    return copy_name(p.name, name, len);
}

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

}  // namespace nbgen

using namespace nbgen;

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
    return param_info(g.params[i], name, len, shape, ndim);
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
