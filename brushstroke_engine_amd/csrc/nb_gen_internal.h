// What the translation units of the C generator share (include/neube_hip.h, "the whole generator"): nb_weight_pack.hip (device weight
// packers), nb_gen_plan.hip (configuration tables, the per-batch planner), nb_generator.hip (the handle and the walk of one pass),
// nb_gen_encoder.hip (the geometry encoder behind the handle) and nb_brush_noise.hip (brush noise sets).  Everything in namespace
// nbgen is internal to the library: hidden visibility, no dynamic symbols.
#pragma once
#include "nb_common.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

namespace nbgen __attribute__((visibility("hidden"))) {

// ---- configuration: parameter and layer tables (config.GeneratorConfig, weights.random_state_dict) ----
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

std::string fmt(const char* f, int a);
void add_param(std::vector<GenParam>& params, const std::string& name, std::initializer_list<int64_t> shape);
// validates and expands a configuration; NB_EINVAL (with nb_last_error) on anything GeneratorConfig would reject or this path
// does not take
int resolve_cfg(const NbGeneratorConfig* c, GenCfg& g);
// the per-batch layer plan (nb_synthesis_plan): every kernel decision of SynthesisNetwork's pass and of the walk
int plan_pass(const GenCfg& g, const NbPlanOptions& o, int n, NbPassPlan* p);
// one parameter of a table as the *_param_info entries return it (every output pointer may be NULL)
int param_info(const GenParam& p, char* name, int len, int64_t shape[4], int* ndim);

// ---- sizes ----
inline size_t h2_bytes(int n, int c, int hw) { return (size_t)n * ((c + 7) / 8) * 2 * hw * 8 * sizeof(_Float16); }
// an h3 / f8 weight container with c_out padded to co_align (64: the generator's modconv kernels, 128: the encoder's conv kernels)
inline size_t h3_weight_bytes(int c_in, int c_out, int co_align) {
    return (size_t)(c_in + 15) / 16 * 9 * 4 * ((c_out + co_align - 1) / co_align * co_align) * 8 * sizeof(_Float16);
}

// ---- launchers of nb_weight_pack.hip that have no entry of their own ----
int pack_h3f8(const float* w, int c_out, int c_in, int co_align, void* out, hipStream_t st);
// p: conv weight, conv bias, BatchNorm weight, bias, running mean, running var; NB_ELAUNCH (no message) if the launch fails
int fold_bn(const float* const* p, int c_out, int per, int ld, float* w_out, float* b_out, hipStream_t st);

// ---- device helpers ----
// The device allocations of one owner: hipMalloc rounded to 256 bytes (NULL for 0 bytes and after a failure, which sticks and is
// reported as "<who>: hipMalloc of ... failed").
struct DeviceAllocs {
    const char* who;
    bool ok = true;
    std::vector<void*> list;
    void* get(size_t bytes) {
        void* p = nullptr;
        if (!ok || bytes == 0) return nullptr;
        if (hipMalloc(&p, (bytes + 255) / 256 * 256) != hipSuccess) {
            ok = false;
            nb_set_error("%s: hipMalloc of %zu bytes failed", who, bytes);
            return nullptr;
        }
        list.push_back(p);
        return p;
    }
    void free_all() {                            // (on the current device; the caller has synchronised it)
        for (void* p : list) (void)hipFree(p);
        list.clear();
    }
};

// makes `device` current (ok: it is) and restores the device that was current on exit
struct DeviceScope {
    int prev = 0;
    const bool have, ok;
    explicit DeviceScope(int device) : have(hipGetDevice(&prev) == hipSuccess), ok(hipSetDevice(device) == hipSuccess) {}
    ~DeviceScope() { if (have) (void)hipSetDevice(prev); }
};

int require_current_device(const NbGenerator* gen, const char* who);

// ---- the walk of one pass (nb_generator.hip) and the encoder's part in it (nb_gen_encoder.hip) ----
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

int gen_walk(NbGenerator* g, const NbGeneratorInputs* in, const NbGeneratorOutputs* out, int n, hipStream_t st, const WalkSink& sink,
             const GeomHook* geom_hook = nullptr, const NbGeneratorStage* stage = nullptr);
int enc_walk(NbGenerator* g, const float* x, int n, hipStream_t st, const NbPassPlan* plan, const WalkSink& sink, size_t* need_ping,
             NbGeneratorInputs* io, unsigned* handed);
// the input rules of a forward pass (`who` prefixes the messages); the geometry features are checked by the caller
int check_forward(NbGenerator* gen, const NbGeneratorInputs* in, int n, const char* who);
int check_modes_and_device(NbGenerator* gen, const NbGeneratorInputs* in, void* stream, const char* who);
// what the forward entries do behind their validation: the pass on a copy of `in` (the encoder fills its geom[] from `patches`
// before the walk reads them; NULL: no encoder in this pass)
int run_forward(NbGenerator* gen, const NbGeneratorInputs* in, const float* patches, const NbGeneratorStage* stage,
                const NbGeneratorOutputs* out, int n, void* stream);

// Where a geometry feature of gch channels goes in the operands of its consumer layer, behind the c_prod channels of the producer:
// the arguments of nb_pack_h2*_part_f32 and of the encoder's hand-off
struct PartPack {
    int c_prod;
    const float* styles;                                 // the consumer's styles of the geometry channels
    int c_in, groups, cg0;                               // the consumer's channels, its 8-channel groups, the first group written
};
PartPack part_pack(const NbGenerator* g, int consumer, int gch);
inline decltype(&nb_pack_h2_part_f32) part_pack_fn(int fmt) { return fmt ? nb_pack_h2f8_part_f32 : nb_pack_h2_part_f32; }

}  // namespace nbgen

// (the three types below are global and of default visibility, as the handles of include/neube_hip.h are)
struct GenLayerDev {
    const float *weight = nullptr, *bias = nullptr, *noise_strength = nullptr, *noise_const = nullptr, *affine_w = nullptr,
                *affine_b = nullptr, *filter = nullptr, *noise_grid = nullptr;
    float *wpk = nullptr, *wsq = nullptr, *noise_lin = nullptr, *noise_const_t = nullptr;
    void *w_h3 = nullptr, *w_f8 = nullptr, *w_h3_up2 = nullptr;
    float *styles = nullptr, *dcoefs = nullptr, *noise = nullptr;
};

// A brush noise set (include/neube_hip.h): per layer noise_const and its transpose in one allocation, and the handle's layer tables
// with noise_const pointing there
struct NbBrushNoise {
    NbGenerator* gen = nullptr;
    float* buf = nullptr;                        // sum over the layers of 2 res^2 floats (each image padded to 256 bytes)
    std::vector<float*> nc, nc_t;                // per layer: [res, res] and its transpose, inside buf
    NbLayerDesc* tables = nullptr;               // as NbGenerator::tables
};

struct NbGenerator {
    nbgen::GenCfg cfg;
    NbPlanOptions opts;              // nb_plan_options_default with the generator's conv_mode
    int n_max = 0, device = 0;
    float act_gain = 0.f;
    nbgen::DeviceAllocs mem{"generator_create"};
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
        nbgen::DeviceAllocs mem{"generator_attach_encoder"};
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
        return nbgen::plan_pass(cfg, o, n, p);
    }
};
