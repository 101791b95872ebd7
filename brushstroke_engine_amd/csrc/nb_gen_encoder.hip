// The geometry encoder behind the generator handle (host only): stroke patches -> the two features (encoder.HipGeometryEncoder.encode,
// driven as SynthesisNetwork._encode_lazy_geometry drives it).  Its kernels live in nb_encoder.hip, its weight fold in
// nb_weight_pack.hip.
#include "nb_gen_internal.h"

namespace nbgen __attribute__((visibility("hidden"))) {
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
    for (const EncLayer& L : kEncLayers) {
        const std::string p = L.prefix;
        add_param(v, p + ".0.weight", {L.c_out, L.c_in, L.k, L.k});
        add_param(v, p + ".0.bias", {L.c_out});
        add_param(v, p + ".1.weight", {L.c_out});
        add_param(v, p + ".1.bias", {L.c_out});
        add_param(v, p + ".1.running_mean", {L.c_out});
        add_param(v, p + ".1.running_var", {L.c_out});
    }
    return v;
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

void enc_free(NbGenerator* g) {
    if (!g->enc.mem.list.empty()) {
        (void)hipDeviceSynchronize();
        g->enc.mem.free_all();
    }
    g->enc = NbGenerator::Encoder();
}

}  // namespace

// HipGeometryEncoder.encode on the handle's workspaces.  Without sink.launch: record the largest ping-pong tensor in *need_ping only.
// Otherwise io->geom[] receives the fp32 features, and feature 1 goes straight into its consumer's operand tensor (pre_h2[1], times
// the consumer's styles) where the plan's encoder hand-off and the patch size allow it: bit 1 of *handed is then set.
int enc_walk(NbGenerator* g, const float* x, int n, hipStream_t st, const NbPassPlan* plan, const WalkSink& sink, size_t* need_ping,
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
    int cur = 0, r = R;
    if (fused) {
        need(h2_bytes(n, kEncLayers[1].c_out, (R / 2) * (R / 2)));
        GEN_TRY(nb_enc_stem_conv3x3_f8(x, E.w50, E.b0, E.preproc, W(0, 1), E.b[0], E.ping[0], narrow(1) ? 0 : fmt, n, R, R,
                                       kEncLayers[1].c_out, slope, st));
        r = R / 2;
    } else {
        need(h2_bytes(n, kEncLayers[0].c_out, R * R));
        GEN_TRY(nb_enc_stem7x7_f32_h2_ex(x, E.w50, E.b0, E.ping[0], fmt, n, R, R, E.preproc, slope, st));
    }
    for (int i = fused ? 1 : 0; i < 4; ++i) {       // three stride-2 stages + 256 -> 32
        const EncLayer& L = kEncLayers[i + 1];
        const int ro = r / L.stride, fin = narrow(i) ? 0 : fmt, fout = narrow(i + 1) ? 0 : fmt;
        need(h2_bytes(n, L.c_out, ro * ro));
        GEN_TRY(nb_enc_conv3x3_ex(E.ping[cur], L.c_in, W(i, fin), E.b[i], nullptr, E.ping[cur ^ 1], nullptr, 0, fout ? L.c_out / 8 : 0, 0, fin,
                                  fout, n, r, r, L.c_out, L.stride, slope, st));
        cur ^= 1;
        r = ro;
    }
    const EncLayer& B = kEncLayers[5];              // 32 -> 16: the bottleneck, feature 0 (fp32)
    const int fin = narrow(4) ? 0 : fmt;
    GEN_TRY(nb_enc_conv3x3_ex(E.ping[cur], B.c_in, W(4, fin), E.b[4], E.feat0, nullptr, nullptr, 0, 0, 0, fin, 0, n, r, r, B.c_out, 1, slope, st));
    GEN_TRY(nb_enc_upsample2x_h2_ex(E.feat0, E.up, fmt, n, B.c_out, r, r, st));
    const EncLayer& D = kEncLayers[6];              // the first decoder stage, 16 -> 256: feature 1
    const int r1 = 2 * r;
    need((size_t)n * D.c_out * r1 * r1 * sizeof(float));
    if (!sink.launch) return NB_OK;
    io->geom[0] = E.feat0;
    const NbGeomPlan& gp = plan->geom[1];
    // the hand-off needs the large-tile epilogue (HipGeometryEncoder.can_handoff) and the consumer's operand tensor of the early pack
    if (gp.encoder_handoff && gp.early_pack && (r1 % 32 == 0 || r1 == 16)) {
        const PartPack pp = part_pack(g, gp.consumer, D.c_out);
        GEN_TRY(nb_enc_conv3x3_ex(g->enc.up, D.c_in, W(5, fmt), E.b[5], nullptr, g->pre_h2[1], pp.styles, pp.c_in, pp.groups, pp.cg0, fmt, gp.fmt,
                                  n, r1, r1, D.c_out, 1, slope, st));
        io->geom[1] = nullptr;
        *handed |= 2u;
    } else {
        float* dec = (float*)E.ping[cur ^ 1];
        GEN_TRY(nb_enc_conv3x3_ex(E.up, D.c_in, W(5, fmt), E.b[5], dec, nullptr, nullptr, 0, 0, 0, fmt, 0, n, r1, r1, D.c_out, 1, slope, st));
        io->geom[1] = dec;
    }
    return NB_OK;
}

}  // namespace nbgen

using namespace nbgen;

extern "C" int nb_encoder_param_count(void) { return (int)(sizeof(kEncLayers) / sizeof(kEncLayers[0])) * kEncParamsPerLayer; }

extern "C" int nb_encoder_param_info(int i, char* name, int len, int64_t shape[4], int* ndim) {
    const std::vector<GenParam> ps = enc_params();
    NB_REQUIRE(i >= 0 && i < (int)ps.size(), "encoder: parameter index %d out of range [0, %d)", i, (int)ps.size());
    return param_info(ps[i], name, len, shape, ndim);
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
    if (const int rc = require_current_device(gen, "generator_attach_encoder")) return rc;
    hipStream_t st = (hipStream_t)stream;
    enc_free(gen);                                   // (a second call replaces the first)
    NbGenerator::Encoder& E = gen->enc;
    DeviceAllocs& keep = E.mem;
    DeviceAllocs temps{keep.who};                    // the folded fp32 weights of the 3x3 layers: freed when this call ends
    auto finish = [&](int code) {
        (void)hipStreamSynchronize(st);
        temps.free_all();
        if (code != NB_OK) enc_free(gen);
        return code;
    };
    const bool f8 = gen->opts.conv_mode == NB_CONV_F8;
    const float* const* P = (const float* const*)enc_params_dev;
    for (int l = 0; l < 7; ++l) {
        const EncLayer& L = kEncLayers[l];
        const int per = L.c_in * L.k * L.k, ld = l == 0 ? 50 : per;
        float* w = (float*)(l == 0 ? keep : temps).get((size_t)L.c_out * ld * sizeof(float));
        float* b = (float*)keep.get((size_t)L.c_out * sizeof(float));
        if (!keep.ok || !temps.ok) return finish(NB_ELAUNCH);
        if (fold_bn(P + l * kEncParamsPerLayer, L.c_out, per, ld, w, b, st)) {
            nb_set_error("generator_attach_encoder: launch of the BatchNorm fold failed");
            return finish(NB_ELAUNCH);
        }
        if (l == 0) {
            E.w50 = w;
            E.b0 = b;
            continue;
        }
        // encoder.pack_enc_weight_h3 / pack_enc_weight_f8: the containers with c_out padded to 128
        const size_t bytes = h3_weight_bytes(L.c_in, L.c_out, 128);
        E.b[l - 1] = b;
        E.w_h3[l - 1] = keep.get(bytes);
        if (f8) E.w_f8[l - 1] = keep.get(bytes);
        if (!keep.ok) return finish(NB_ELAUNCH);
        int rc = nb_pack_conv_weight_h3_dev(w, L.c_out, L.c_in, 128, 0, E.w_h3[l - 1], st);
        if (!rc && f8) rc = pack_h3f8(w, L.c_out, L.c_in, 128, E.w_f8[l - 1], st);
        if (rc) return finish(rc);
    }
    // workspaces: the largest each gets at any batch up to n_max (below batch 8, and always for h3 / f32 generators, the stem writes the
    // 64-channel full-resolution tensor that the fused f8 launch never creates)
    size_t need_ping = 0;
    for (int n = 1; n <= gen->n_max; ++n) enc_walk(gen, nullptr, n, st, nullptr, WalkSink(), &need_ping, nullptr, nullptr);
    const int R = gen->cfg.R;
    E.ping[0] = keep.get(need_ping);
    E.ping[1] = keep.get(need_ping);
    E.feat0 = (float*)keep.get((size_t)gen->n_max * 16 * (R / 8) * (R / 8) * sizeof(float));
    E.up = keep.get(h2_bytes(gen->n_max, 16, (R / 4) * (R / 4)));
    if (!keep.ok) return finish(NB_ELAUNCH);
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
    if (const int rc = check_forward(gen, in, n, "generator_forward_geom")) return rc;
    if (const int rc = check_modes_and_device(gen, in, stream, "generator_forward_geom")) return rc;
    return run_forward(gen, in, geom, nullptr, out, n, stream);
}
