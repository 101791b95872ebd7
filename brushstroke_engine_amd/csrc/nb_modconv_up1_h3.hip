// Split-f16 ("h3") modulated 3x3 convolution, up = 1, for gfx950: fp32-accurate products on the f16 matrix
// cores at ~5x the fp32-MFMA rate.
//
// Every fp32 operand v is carried as two halves  v = hi + lo,  hi = f16(v), lo = f16(v - hi)  (22 significant
// bits); a product is evaluated as  x*w ~= xh*wh + xl*wh + xh*wl  with three v_mfma_f32_32x32x16_f16 (products
// of two f16 are exact in fp32, accumulation is fp32); the dropped xl*wl term is 2^-22 relative.  End to end
// (14 stacked layers, R=128) this differs from the all-fp32 evaluation by 5e-6 on pixels, against 3e-3 for a
// plain single-f16 evaluation (tools/split_precision_check.py) -- far inside the 1e-3 parity budget.
//
// The style modulation is applied by the PRODUCER of the activation tensor (x * s[n,c] is what gets split and
// stored), so the weights are static and pre-split once at load time; the demodulation d[n,o] stays in the
// fp32 epilogue.  Reference arithmetic: training/networks.py:67-76 (non-fused form of modulated_conv2d).
//
// Activation format "H2":  _Float16 [N][C/8][2 (hi, lo)][H][W][8]   -- 8 channels of one pixel = 16 bytes =
// one lane's MFMA fragment (k = 8 consecutive channels), so halo-tile rows are contiguous 16-byte slots in HBM
// and LDS and every staging transfer is a global_load_lds_dwordx4 (no VGPRs, no alignment games).
// Weight format:  _Float16 [C_in/16][ky 3][kx 3][cg 2][hi/lo 2][C_out_ld][8].
//
// Workgroup = 8 waves as MW (c_out) x 8/MW (pixels), wave tile 64 c_out x 64 pixels (2x2 MFMA tiles, 64
// accumulator registers), i.e. 128 x 256 (MW=2) or 64 x 512 (MW=1) per workgroup; pixel blocks are image rows
// of 32.  K loop: 16-channel chunks x 3 tap rows; the weights of one (chunk, tap row) form a 4-deep LDS ring,
// the activation halo tile of a chunk is double buffered; counted vmcnt + raw s_barrier keep 2 sub-chunks of
// LDS-DMA in flight behind the MFMAs.
#include "nb_h3_launch.h"
#include "nb_torgb.h"

struct H3Params {
    const _Float16* x;      // H2 [n][c8][2][H][W][8], already multiplied by this layer's styles
    const _Float16* wts;    // [nchunks][3][3][2][2][co_ld][8]
    const float* dcoefs;    // [n][c_out]
    const float* noise;     // [n or 1][H][W] or null
    NbNoiseSrcDev nsrc;     // nsrc.const_t != null: the noise is computed here (NbNoiseSrc), `noise` is null
    const float* bias;      // [c_out]
    float* y;               // fp32 NCHW [n][c_out][H][W] or null
    const float* zeros;
    long long noise_stride_n;
    int c8, nchunks, c_out, co_ld, h, w;
    int tiles_x, tiles_y, slices, dbg, stagger_ticks;
    int items, items_x;            // persistent workgroups (8-wave kernel): items = tiles x slices x samples of the launch, items_x = per sample
    float alpha, gain, clamp;
    unsigned long long* tstamps;   // debug: per-workgroup phase timestamps (nb_debug_set_timestamps), else null
    // H2 output (y == null): the result, multiplied by the CONSUMER's styles, goes straight into the consumer's H2
    // input tensor [n][c8_next][2][H][W][8] (channel groups 0 .. c_out/8-1), so no separate packing pass is needed
    _Float16* yh2;
    const float* next_styles;      // [n][next_stride]
    int next_stride, c8_next;
    int out_f8;                    // H2 output in the "f8" operand format (the consumer's corrections run on fp8 MFMAs)
    // fused triad ToRGB (last layer; the workgroup holds all c_out channels of its pixels): tg.c != 0 enables it,
    // y may then be null (the fp32 activations are only needed when somebody taps them)
    TorgbParams tg;
};

unsigned long long* g_tstamps = nullptr;
int g_tstamps_cap = 0;
// Debug hook (not part of the product ABI): phase timestamps [workgroup][8] of the next h3 launches, s_memrealtime ticks
extern "C" void nb_debug_set_timestamps(void* buf, int capacity_workgroups) { g_tstamps = (unsigned long long*)buf; g_tstamps_cap = capacity_workgroups; }

// Activation of the split-f16 kernels: lrelu(g (a d + noise + bias)) clamped, with the gain g > 0 folded into the three
// addends (lrelu(g t) = g lrelu(t)).  Every output path of a kernel -- fp32, H2, f8 -- evaluates exactly this expression
// (dg = d g, nbg = bias g + noise g), so that a fused hand-off equals the fp32 output packed afterwards bit for bit.
__device__ __forceinline__ float nb_h3_act(float a, float dg, float nbg, float alpha, float clampv) {
    const float t = __builtin_fmaf(a, dg, nbg);
    // lrelu = max(t, alpha t) for 0 <= alpha <= 1 (the launchers check); clampv = +inf for "no clamp"
    return __builtin_amdgcn_fmed3f(__builtin_amdgcn_fmed3f(t, t * alpha, __builtin_inff()), -clampv, clampv);
}

// (the hand-off epilogue of the up=1 kernels, nb_up1_handoff_epilogue, lives in nb_h3_common.h: the geometry encoder's conv kernel uses it too)

// NBW_ = 32-pixel rows per wave: 2 for throughput, 1 (half the pixels per workgroup, twice the workgroups) when the
// launch would otherwise leave most of the chip idle - the batch-1 / interactive configuration.
// V2: the K loop in the form of modconv3x3_up2v_kernel (nb_modconv_up2v.hip) -- LDS-DMA from inline assembly
// (counted lgkmcnt waits), the step's barrier in front of its last two MFMA groups with the next step's first operands read under
// them, fragment reads and DMA pieces dealt out between the MFMAs.  Same per-accumulator order of products: bit-identical.
// F6 (with F8 and V2): the "f6" operand format (nb_h3_common.h) -- the K loop of the f8 V2 form with fp6 correction products.
// PP (with F8 and V2, round 5): the f8 K loop as a PING-PONG of the two waves of a SIMD (waves w and w + 4): a step is a LOAD segment -- all
// of the step's fragment reads and its LDS-DMA pieces, no matrix instruction -- and a COMPUTE segment -- the step's 18 MFMAs back to back,
// every operand in registers --, waves 4-7 run one segment behind waves 0-3, a barrier after every segment: while one wave of a SIMD
// computes, its partner loads.  Same per-accumulator order of products as the other f8 loops: bit-identical.
// HO (with PPK, round 6): "hi only" -- the ping-pong f8 loop WITHOUT its correction products (plain single-f16 evaluation, ~3e-3 from
// fp32: Generator(conv_mode="f16"), a timing data point at the reference's shipped precision, not a parity mode; see modconv3x3_up2v_kernel).
// PERSIST = false: the same body WITHOUT the tile loop (item_next is the list's end at compile time: no next tile, no prefetch, no carried state;
// 208-210 instead of 256 registers, no spills) -- one workgroup per tile as until round 5.  DEFAULT for the ping-pong launches: against round 5's
// kernels linked into the same library (profiles/r06_ab_variants*.txt) the persistent form is 4.4 % SLOWER at 64 channels (b256.conv1 + ToRGB:
// 0.347 -> 0.362 ms per step), equal at 128, and costs the three-streams schedule 1.4 % -- while its own "one workgroup per tile" switch,
// which kept the loop, had said -3 ... -4 %.  The persistent instantiation stays behind nb_debug_set_up1_persistent(1).
template <int MW, bool F8 = false, int NBW_ = 2, bool V2 = false, bool F6 = false, bool PPK = false, bool HO = false, bool PERSIST = true>
__global__ __launch_bounds__(512) void modconv3x3_up1_h3_kernel(const H3Params p) {
    static_assert(!HO || PPK, "the hi-only form is a variant of the ping-pong f8 loop");
    static_assert(!F6 || (F8 && V2), "the f6 form is a variant of the software-pipelined f8 loop");
    static_assert(!PPK || (F8 && V2 && !F6), "the ping-pong form is a variant of the software-pipelined f8 loop");
    NB_TSTAMP(0);
    if (p.out_f8) nb_set_fp16_ovfl();             // f8 hand-off: the fp8 (and f16) conversions saturate
    nb_stagger(p.stagger_ticks, 256);
    constexpr int NW = 8, NWN = NW / MW;          // waves along pixels
    constexpr int MB = 2, NBW = NBW_;             // 32x32 MFMA tiles per wave: 64 c_out x 64 (32) pixels
    constexpr int CO_WG = MW * 64, TH = NWN * NBW, TWP = 34;     // tile rows (32 pixels each), halo tile width
    constexpr int SLOTS = (TH + 2) * TWP;         // 16-byte slots of one (cgroup, hi/lo) plane of the halo tile
    constexpr int PP = (SLOTS + 63) / 64;         // 1-KiB DMA pieces per plane
    constexpr int XPL = PP * 64;                  // slots reserved per plane
    constexpr int NXP = 4 * PP, NXPW = (NXP + NW - 1) / NW;      // activation pieces per chunk / per wave
    constexpr int WSLOTS = 12 * CO_WG;            // slots of one (chunk, tap row) weight sub-chunk: [kx][cg][hl][c_out]
    constexpr int NWP = WSLOTS / 64, NWPW = (NWP + NW - 1) / NW;
    constexpr int WST = 4;                        // weight ring depth
    static_assert(WST == 4, "the ring indices below are written as (t & 3)");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_h3[];
    h8* xbuf = reinterpret_cast<h8*>(smem_h3);                    // [2][4 planes][XPL]
    h8* wring = xbuf + 2 * 4 * XPL;                               // [WST][WSLOTS]

    const int tid = threadIdx.x;
    const int lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6), lh = lane >> 5, l31 = lane & 31;
    const int wm = wv / NWN, wn = wv - wm * NWN;  // wave coordinates (c_out, pixel rows)
    const int H = p.h, W = p.w;
    // PERSISTENT workgroups (round 6): gridDim.x = min(items, CUs); workgroup w renders items w, w + gridDim.x, ... of the list
    // [sample][tile][c_out slice] (p.items of them, p.items_x per sample), and the NEXT tile's prologue -- its halo tile and first three
    // weight sub-chunks, ~4 us of LDS-DMA round trip -- is issued BEFORE this tile's epilogue, which works straight from the
    // accumulators (hand-off / fused ToRGB outputs) and leaves the staging LDS alone.
    // XCD-aware order (as in the up=2 kernels): hardware workgroup ids go round-robin to the 8 XCDs, each with its own L2;
    // renumbered, an XCD works on a contiguous run of a sample's row-major tile list -- whole tile rows -- so that the halo columns
    // and rows neighbouring tiles share are L2 hits instead of second HBM reads (gridDim.x is a multiple of 8 whenever the per-sample
    // list is, so a workgroup's items keep to its XCD)
    typedef const __attribute__((address_space(4))) H3Params* kparams_t;
    auto fresh_params = [&]() -> kparams_t {           // (per-tile reads of the launch parameters: not carried in registers across the K loop)
        kparams_t q = (kparams_t)__builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(q));
        return q;
    };
    int n = 0, y0 = 0, x0 = 0, co0 = 0;
    bool sample_lead = false;                      // exactly one item per sample: it writes the sample's ToRGB colors
    const size_t HW8 = (size_t)H * W * 8;
    auto tile_coords = [&](unsigned l) {
        kparams_t q_ = fresh_params();
        const unsigned gx = (unsigned)q_->items_x;
        unsigned b = l % gx;
        sample_lead = b == 0;
        const unsigned nn = l / gx;
        if (gx % 8 == 0 && gridDim.x % 8 == 0 && !(q_->dbg & 8)) b = (b & 7) * (gx >> 3) + (b >> 3);
        const int slice = b % q_->slices; b /= q_->slices;
        const int tile_x = b % q_->tiles_x; const int tile_y = b / q_->tiles_x;
        n = __builtin_amdgcn_readfirstlane((int)nn); y0 = __builtin_amdgcn_readfirstlane(tile_y * TH);
        x0 = __builtin_amdgcn_readfirstlane(tile_x * 32); co0 = __builtin_amdgcn_readfirstlane(slice * CO_WG);
    };
    unsigned item = __builtin_amdgcn_readfirstlane(blockIdx.x);
    const unsigned total = (unsigned)p.items;
    tile_coords(item);

    // epilogue operands are fetched at the top of a tile, under the prologue DMA: per-channel demodulation / bias into LDS, the
    // lane's noise values into registers (fetching them in the epilogue costs ~10 us of exposed latency per tile)
    __shared__ __attribute__((aligned(16))) float s_dco[CO_WG], s_bias[CO_WG], s_nst[CO_WG];
    __shared__ __attribute__((aligned(16))) float s_tw[3 * CO_WG];
    __shared__ float s_tcol[9], s_tcol01[9];
    float nzr[NBW];
    int tg_n = -1;                                 // sample whose ToRGB tables (weights x styles) are in LDS
    auto load_tile_tables = [&]() {
        kparams_t q_ = fresh_params();
        if (tid < CO_WG) {
            const int co = co0 + tid, c_out = q_->c_out;
            s_dco[tid] = co < c_out ? q_->dcoefs[(size_t)n * c_out + co] : 0.f;
            s_bias[tid] = co < c_out ? q_->bias[co] : 0.f;
            s_nst[tid] = (q_->yh2 && co < c_out) ? q_->next_styles[(size_t)n * q_->next_stride + co] : 0.f;
        }
        // (weights x styles of the sample into LDS; the sample's lead item also writes its colors -- every item of the lead's sample
        //  that this workgroup renders goes through here with the tables in place, so the lead must not be skipped)
        if (p.tg.c && (n != tg_n || sample_lead)) { nb_torgb_setup(p.tg, n, s_tw, s_tcol, s_tcol01, tid, 512, sample_lead); tg_n = n; }
        const float* noise = q_->noise;
#pragma unroll
        for (int nb = 0; nb < NBW; ++nb)
            nzr[nb] = noise ? noise[(size_t)n * q_->noise_stride_n + (size_t)(y0 + wn * NBW + nb) * W + x0 + l31] : 0.f;
        if (q_->nsrc.const_t) {
            // the lane's pixels (row y0 + wn NBW + nb, column x0 + l31): column parameters once, row parameters per row
            const NbNoiseSrcDev nsrc{q_->nsrc.const_t, q_->nsrc.lin, q_->nsrc.strength, q_->nsrc.norm_pos, q_->nsrc.positions, q_->nsrc.res, q_->nsrc.img_res};
            float np0, np1, wy0, wy1;
            int sy0;
            nb_noise_np(nsrc, n, np0, np1);
            nb_noise_axis(nsrc, x0 + l31, np1, sy0, wy0, wy1);
            const float strength = nsrc.strength[0];
#pragma unroll
            for (int nb = 0; nb < NBW; ++nb) {
                float wx0, wx1;
                int sx0;
                nb_noise_axis(nsrc, y0 + wn * NBW + nb, np0, sx0, wx0, wx1);
                nzr[nb] = nb_noise_value(nsrc, strength, sx0, wx0, wx1, sy0, wy0, wy1);
            }
        }
    };

    // ---- DMA descriptors of this wave's activation pieces ----
    int xsp[NXPW], xpl[NXPW], xdst[NXPW];
    const _Float16* xn = p.x;
#pragma unroll
    for (int i = 0; i < NXPW; ++i) {
        int q = i * NW + wv;
        q = q < NXP ? q : NXP - 1;
        const int pl = q / PP, part = q - pl * PP;      // pl = cg_local*2 + hi/lo
        xpl[i] = __builtin_amdgcn_readfirstlane(pl);
        xdst[i] = __builtin_amdgcn_readfirstlane(pl * XPL + part * 64);
    }
    // the CURRENT tile's per-lane sources (y0, x0, n as tile_coords left them; through an opaque statement: recomputed per tile)
    auto piece_offsets = [&]() {
        int y0_ = y0, x0_ = x0, lane_ = lane;
        asm volatile("" : "+v"(y0_), "+v"(x0_), "+v"(lane_));
        y0_ = __builtin_amdgcn_readfirstlane(y0_); x0_ = __builtin_amdgcn_readfirstlane(x0_);
        kparams_t q_ = fresh_params();
        xn = q_->x + (size_t)n * q_->c8 * 2 * HW8;
#pragma unroll
        for (int i = 0; i < NXPW; ++i) {
            int q = i * NW + wv;
            q = q < NXP ? q : NXP - 1;
            const int part = q % PP;
            const int e = part * 64 + lane_;
            xsp[i] = -1;
            if (e < SLOTS) {
                const int r = e / TWP, c = e - r * TWP;
                const int gy = y0_ - 1 + r, gx = x0_ - 1 + c;
                if (gy >= 0 && gy < H && gx >= 0 && gx < W) xsp[i] = (gy * W + gx) * 8;
            }
        }
    };
    piece_offsets();
    auto issue_x = [&](int c, h8* dst) {
#pragma unroll
        for (int i = 0; i < NXPW; ++i) {
            const int cg = 2 * c + (xpl[i] >> 1);
            const _Float16* src = reinterpret_cast<const _Float16*>(p.zeros);
            if (xsp[i] >= 0 && cg < p.c8) src = xn + (size_t)(4 * c + xpl[i]) * HW8 + xsp[i];
            __builtin_amdgcn_global_load_lds(NB_GLOBAL_PTR(src), NB_LDS_PTR(dst + xdst[i]), 16, 0, 0);
        }
    };
    auto issue_w = [&](int t, h8* dst) {          // t = chunk*3 + ky
#pragma unroll
        for (int i = 0; i < NWPW; ++i) {
            int q = i * NW + wv;
            q = q < NWP ? q : NWP - 1;
            const int e = q * 64 + lane;
            const int row = e / CO_WG, j = e - row * CO_WG;     // row = kx*4 + cg*2 + hl
            const _Float16* src = p.wts + (((size_t)t * 12 + row) * p.co_ld + co0 + j) * 8;
            __builtin_amdgcn_global_load_lds(NB_GLOBAL_PTR(src), NB_LDS_PTR(dst + q * 64), 16, 0, 0);
        }
    };

    f32x16 acc[MB][NBW];

    const int NC = p.nchunks, T = NC * 3;
    auto clampt = [&](int t) { return t < T ? t : T - 1; };
    // V2: the same pieces from inline assembly (a builtin LDS-DMA anywhere in the kernel pins every fragment-read wait at
    // lgkmcnt(0), see nb_lds_dma16): per-lane source of chunk 0 + per-chunk stride (0 for out-of-image slots: the zero page),
    // weights as a uniform base per step + a lane offset
    const unsigned lds0_v2 = (unsigned)(uintptr_t)NB_LDS_PTR(smem_h3);
    const char* xs0_v2[NXPW];
    unsigned xst_v2[NXPW], wof_v2[NWPW];
    auto piece_sources_v2 = [&]() {
        kparams_t q_ = fresh_params();
        int c0_ = co0, lane_ = lane;
        asm volatile("" : "+v"(c0_), "+v"(lane_));
        c0_ = __builtin_amdgcn_readfirstlane(c0_);
#pragma unroll
        for (int i = 0; i < NXPW; ++i) {
            const bool in = xsp[i] >= 0;
            xs0_v2[i] = in ? reinterpret_cast<const char*>(xn + (size_t)xpl[i] * HW8 + xsp[i]) : reinterpret_cast<const char*>(q_->zeros);
            xst_v2[i] = in ? (unsigned)(4 * HW8 * 2) : 0u;
        }
#pragma unroll
        for (int i = 0; i < NWPW; ++i) {
            int q = i * NW + wv;
            q = q < NWP ? q : NWP - 1;
            const int e = q * 64 + lane_;
            const int row = e / CO_WG, j = e - row * CO_WG;
            wof_v2[i] = (unsigned)(((size_t)row * q_->co_ld + c0_ + j) * 16);
        }
    };
    if constexpr (V2) piece_sources_v2();
    const size_t wstep_v2 = (size_t)12 * p.co_ld * 16;                 // bytes of one (chunk, tap row) weight sub-chunk
    constexpr int WRING_SLOT0 = 2 * 4 * XPL;
    auto issue_x_v2 = [&](auto ii, int c, int buf) {                   // piece ii of chunk c's halo tile into activation buffer buf
        constexpr int i = decltype(ii)::value;
        nb_lds_dma16_m(xs0_v2[i] + (size_t)c * xst_v2[i], lds0_v2 + (unsigned)(buf * 4 * XPL + xdst[i]) * 16u, ~0ull);
    };
    auto issue_w_v2 = [&](auto ii, int t, int slot) {                  // piece ii of weight sub-chunk t into ring slot `slot`
        constexpr int i = decltype(ii)::value;
        int q = i * NW + wv;
        q = q < NWP ? q : NWP - 1;
        nb_lds_dma16_s(reinterpret_cast<const char*>(p.wts) + (size_t)t * wstep_v2, wof_v2[i], lds0_v2 + (unsigned)(WRING_SLOT0 + slot * WSLOTS + q * 64) * 16u);
    };
    // a tile's prologue: chunk 0's halo tile and the first three weight sub-chunks
    auto prologue_issue = [&]() {
        if constexpr (V2) {
            nb_static_for<0, NXPW>([&](auto i) { issue_x_v2(i, 0, 0); });
            nb_static_for<0, NWPW>([&](auto i) { issue_w_v2(i, 0, 0); });
            nb_static_for<0, NWPW>([&](auto i) { issue_w_v2(i, clampt(1), 1); });
            nb_static_for<0, NWPW>([&](auto i) { issue_w_v2(i, clampt(2), 2); });
        } else {
            issue_x(0, xbuf);
            issue_w(0, wring);
            issue_w(clampt(1), wring + WSLOTS);
            issue_w(clampt(2), wring + 2 * WSLOTS);
        }
    };
    NB_TSTAMP(5);                              // (the hand-off epilogues leave slot 5 free: time that passes before the first LDS-DMA piece goes out)
    prologue_issue();
  for (;;) {                                   // one iteration per tile of this workgroup (see PERSISTENT above)
#undef NB_TSTAMP
#define NB_TSTAMP(k) do { if (p.tstamps && threadIdx.x == 0) { unsigned it_ = item; asm volatile("" : "+v"(it_)); p.tstamps[(size_t)it_ * 8 + (k)] = __builtin_amdgcn_s_memrealtime(); } } while (0)
    load_tile_tables();
#pragma unroll
    for (int mb = 0; mb < MB; ++mb)
#pragma unroll
        for (int nb = 0; nb < NBW; ++nb)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mb][nb][r] = 0.f;
    // step 0 needs the halo tile and sub-chunk 0 only: sub-chunks 1 and 2 may still be in flight (the loop's invariant)
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * NWPW) : "memory");
    __builtin_amdgcn_s_barrier();
    NB_TSTAMP(1);

    // fragment addresses (in 16-byte slots)
    const int a_base = lh * 2 * CO_WG + wm * 64 + l31;           // + kx*4*CO_WG + hl*CO_WG + mb*32
    const int b_base = lh * 2 * XPL + (wn * NBW) * TWP + l31;    // + hl*XPL + (nb + ky)*TWP + kx

    unsigned long long t_dma = 0, t_bar = 0;
    const unsigned long long t_loop0 = p.tstamps ? __builtin_amdgcn_s_memtime() : 0;
    if constexpr (F6) {
        // ---- f6 operands: the f8 loop below with the correction products on fp6 MFMAs (32 instead of 64 cycles each) -----------
        // A lane's 32 K values of a correction instruction = ONE tap of ONE pixel / c_out, both terms (one block scale per lane):
        // lane half 0 takes tap 0 of the pair (0, 1), lane half 1 tap 1 -- the lo-slot addresses are per lane --, and its operand is
        // the chunk's two lo slots: six registers of fields (read as 16 + 8 bytes) and the scale dword (4 bytes) = the instruction's
        // scale operand.  Tap 2 has no partner in its step: its corrections run alone every step, lane half 1 multiplying a zero slot
        // (weights side).  Per step and tile 3 f16 + 2 fp6 MFMAs = 160 cycles (f8: 3 x 32 + 1.5 x 64 = 192).  Step t:
        //   part A:  tap 2 main (t-1) | tap-2 corrections (t-1) | tap 0 (t)      fillers: the step's LDS-DMA pieces, its tap-2 fragments
        //   wait (counted) + barrier
        //   part B:  tap 1 (t) | corrections 0 + 1 (t)                           fillers: hi fragments of taps 0, 1 of step t+1;
        //            behind the last fp6 MFMA the lo slots of step t+1
        // Measured (profiles/r05_f6_ab.txt): not faster than the f8 loop -- neither loop is bound by the matrix pipe.
#define NB_SB __builtin_amdgcn_sched_barrier(0)
#define NB_Q(v, q, src) { const i32x4 t_ = __builtin_bit_cast(i32x4, (src)); v[4 * (q)] = t_[0]; v[4 * (q) + 1] = t_[1]; v[4 * (q) + 2] = t_[2]; v[4 * (q) + 3] = t_[3]; }
        __shared__ __attribute__((aligned(16))) h8 s_zero6[1];
        if (tid == 0) s_zero6[0] = h8{};
        __builtin_amdgcn_s_barrier();
        h8 ah0[MB], ah1[MB], ah2[MB], bh0[NBW], bh1[NBW], bh2[NBW];
        v6i al01[MB], bl01[NBW], al2[MB], bl2[NBW];
        int sa01[MB], sb01[NBW], sa2[MB], sb2[NBW];
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) { ah2[mb] = h8{}; al2[mb] = v6i{}; al01[mb] = v6i{}; sa01[mb] = 0; sa2[mb] = 0; }
#pragma unroll
        for (int nb = 0; nb < NBW; ++nb) { bh2[nb] = h8{}; bl2[nb] = v6i{}; bl01[nb] = v6i{}; sb01[nb] = 0; sb2[nb] = 0; }
        constexpr int NM = MB * NBW, NF = MB + NBW;
        const int a6 = wm * 64 + l31 + CO_WG, a6_01 = a6 + lh * 4 * CO_WG;          // slot (cg 0, lo) of tap 0 / of the lane's tap; (cg 1, lo) = + 2 CO_WG
        const int b6 = (wn * NBW) * TWP + l31 + XPL, b6_01 = b6 + lh;                 // plane (cg 0, lo); (cg 1, lo) = + 2 XPL
        auto rd_hi = [&](auto i_, h8 (&a)[MB], h8 (&b)[NBW], const h8* wb, const h8* xb, int ky, int kx) {
            constexpr int i = decltype(i_)::value;
#ifdef NB_ABL6_NOREAD
            return;
#endif
            if constexpr (i < MB) a[i] = wb[a_base + kx * 4 * CO_WG + i * 32];
            else b[i - MB] = xb[b_base + (i - MB + ky) * TWP + kx];
        };
        // an fp6 operand: 16 + 8 bytes of fields, 4 bytes of scale (volatile: the compiler must not fuse them into a 16-byte read, which
        // cannot land across the end of the six-register operand)
        auto rd6 = [](v6i& t, int& sc, const h8* slot0, const h8* slot1) {
            // (explicit LDS address space: through a generic pointer the volatile reads become flat loads, which count in vmcnt)
            typedef const volatile __attribute__((address_space(3))) int* lds_vint;
            typedef const volatile __attribute__((address_space(3))) i32x2* lds_vint2;
            const i32x4 q0 = __builtin_bit_cast(i32x4, *slot0);
            const i32x2 q1 = *(lds_vint2)NB_LDS_PTR(slot1);
            sc = ((lds_vint)NB_LDS_PTR(slot1))[2];
            t[0] = q0[0]; t[1] = q0[1]; t[2] = q0[2]; t[3] = q0[3]; t[4] = q1[0]; t[5] = q1[1];
        };
        // fragment i of the pair (0, 1) -- the lane's own tap -- or of the lone tap 2 (weights of lane half 1: the zero slot)
        auto rd_lo01 = [&](auto i_, const h8* wb, const h8* xb, int ky) {
            constexpr int i = decltype(i_)::value;
#ifdef NB_ABL6_NOREAD
            return;
#endif
            if constexpr (i < MB) { const h8* s_ = wb + a6_01 + i * 32; rd6(al01[i], sa01[i], s_, s_ + 2 * CO_WG); }
            else { const h8* s_ = xb + b6_01 + (i - MB + ky) * TWP; rd6(bl01[i - MB], sb01[i - MB], s_, s_ + 2 * XPL); }
        };
        auto rd_lo2 = [&](auto i_, const h8* wb, const h8* xb, int ky) {
            constexpr int i = decltype(i_)::value;
#ifdef NB_ABL6_NOREAD
            return;
#endif
            if constexpr (i < MB) { const h8* s_ = wb + a6 + 8 * CO_WG + i * 32; rd6(al2[i], sa2[i], lh ? &s_zero6[0] : s_, lh ? &s_zero6[0] : s_ + 2 * CO_WG); }
            else { const h8* s_ = xb + b6 + (i - MB + ky) * TWP + 2; rd6(bl2[i - MB], sb2[i - MB], s_, s_ + 2 * XPL); }
        };
        auto group = [&](auto nfill_, auto&& mf, auto&& ff) {
            constexpr int NFILL = decltype(nfill_)::value;
            nb_static_for<0, NM>([&](auto k_) {
                constexpr int k = decltype(k_)::value;
                mf(std::integral_constant<int, k / NBW>{}, std::integral_constant<int, k % NBW>{});
                NB_SB;
                nb_static_for<0, NFILL>([&](auto i_) {
                    constexpr int i = decltype(i_)::value;
                    if constexpr (i * NM / (NFILL > 0 ? NFILL : 1) == k) ff(i_);
                });
                NB_SB;
            });
        };
        auto mf_f16 = [&](h8 (&a)[MB], h8 (&b)[NBW]) {
            return [&](auto mb_, auto nb_) {
                constexpr int mb = decltype(mb_)::value, nb = decltype(nb_)::value;
#ifdef NB_ABL6_NOMFMA
                return;
#endif
                acc[mb][nb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[mb], b[nb], acc[mb][nb], 0, 0, 0);
            };
        };
        auto wide = [](const v6i& t) { return i32x8{t[0], t[1], t[2], t[3], t[4], t[5], 0, 0}; };
        auto mf_fp6 = [&](v6i (&a)[MB], int (&sa6)[MB], v6i (&b)[NBW], int (&sb6)[NBW]) {
            return [&](auto mb_, auto nb_) {
                constexpr int mb = decltype(mb_)::value, nb = decltype(nb_)::value;
#if defined(NB_ABL6_NOFP6) || defined(NB_ABL6_NOMFMA)
                return;
#endif
                acc[mb][nb] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(wide(a[mb]), wide(b[nb]), acc[mb][nb], 2, 2, 0, sa6[mb], 0, sb6[nb]);
            };
        };
        auto step = [&](auto ky_, int t, int c) {
            constexpr int KY = decltype(ky_)::value;
            constexpr int NDMA = NWPW + (KY == 0 ? NXPW : 0);
            const h8* xb = xbuf + (c & 1) * 4 * XPL;
            const h8* wb = wring + (t & 3) * WSLOTS;
            const int tn = t + 1, cn = KY == 2 ? c + 1 : c;
            constexpr int KYN = KY == 2 ? 0 : KY + 1;
            const h8* xbn = xbuf + (cn & 1) * 4 * XPL;
            const h8* wbn = wring + (tn & 3) * WSLOTS;
            const int t3 = clampt(t + 3), c1 = c + 1 < NC ? c + 1 : NC - 1;
            auto dma = [&](auto i_) {
                constexpr int i = decltype(i_)::value;
#ifdef NB_ABL6_NODMA
                return;
#endif
                if constexpr (i < NWPW) issue_w_v2(i_, t3, (t + 3) & 3);
                else issue_x_v2(std::integral_constant<int, i - NWPW>{}, c1, (c + 1) & 1);
            };
            NB_SB;
            // part A
            group(std::integral_constant<int, NDMA>{}, mf_f16(ah2, bh2), dma);                       // tap 2 of step t-1
            group(std::integral_constant<int, NF>{}, mf_fp6(al2, sa2, bl2, sb2),                      // its corrections
                  [&](auto i_) { rd_hi(i_, ah2, bh2, wb, xb, KY, 2); });
            group(std::integral_constant<int, NF>{}, mf_f16(ah0, bh0), [&](auto i_) { rd_lo2(i_, wb, xb, KY); });       // tap 0
#ifdef NB_ABL6_NODMA
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
#else
            if constexpr (KY == 2) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(2 * NWPW) : "memory");
            else asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(2 * NWPW + NXPW) : "memory");
#endif
            NB_SB;
            // part B
            group(std::integral_constant<int, NF>{}, mf_f16(ah1, bh1),                                // tap 1
                  [&](auto i_) { rd_hi(i_, ah0, bh0, wbn, xbn, KYN, 0); });
            group(std::integral_constant<int, NF>{}, mf_fp6(al01, sa01, bl01, sb01),                  // corrections of taps 0 + 1
                  [&](auto i_) { rd_hi(i_, ah1, bh1, wbn, xbn, KYN, 1); });
            nb_static_for<0, NF>([&](auto i_) { rd_lo01(i_, wbn, xbn, KYN); });
            NB_SB;
        };
        // operands of step 0
        nb_static_for<0, NF>([&](auto i_) { rd_hi(i_, ah0, bh0, wring, xbuf, 0, 0); });
        nb_static_for<0, NF>([&](auto i_) { rd_hi(i_, ah1, bh1, wring, xbuf, 0, 1); });
        nb_static_for<0, NF>([&](auto i_) { rd_lo01(i_, wring, xbuf, 0); });
        using K0 = std::integral_constant<int, 0>; using K1 = std::integral_constant<int, 1>; using K2 = std::integral_constant<int, 2>;
        for (int c = 0; c < NC; ++c) { step(K0{}, 3 * c, c); step(K1{}, 3 * c + 1, c); step(K2{}, 3 * c + 2, c); }
        NB_SB;
        // the last step's tap 2 and its corrections
        nb_static_for<0, NM>([&](auto k_) { constexpr int k = decltype(k_)::value; mf_f16(ah2, bh2)(std::integral_constant<int, k / NBW>{}, std::integral_constant<int, k % NBW>{}); NB_SB; });
        nb_static_for<0, NM>([&](auto k_) { constexpr int k = decltype(k_)::value; mf_fp6(al2, sa2, bl2, sb2)(std::integral_constant<int, k / NBW>{}, std::integral_constant<int, k % NBW>{}); NB_SB; });
    } else if constexpr (F8 && V2) {
        // ---- f8 operands, software-pipelined over the barrier ------------------------------------------------------
        // Step t = (chunk c, tap row ky) multiplies, per accumulator tile and in this order: tap 2 of step t-1 (f16), on even t
        // the tap-2 corrections of steps t-2 and t-1 (ONE fp8 K = 64), tap 0 (f16), tap 1 (f16), the corrections of taps 0 + 1
        // (fp8) -- the order of the loop below.  What differs is where the barrier stands and when operands are read:
        //   part A:  tap 2 (t-1) | [tap-2 corrections] | tap 0 (t)      fillers: the step's LDS-DMA pieces, its tap-2 fragments
        //   wait (counted) + barrier: every wave has read ALL of stage t; stage t+1 has landed
        //   part B:  tap 1 (t) | corrections 0 + 1 (t)                  fillers: hi fragments of taps 0, 1 of step t+1;
        //            behind the last fp8 MFMA the lo halves of step t+1 (their tuples were its operands)
        // so no step opens with a burst of sixteen reads behind a barrier that both waves of a SIMD reach together.
        // All compile-time: the loop body is two chunks = six steps (tap row and the parity that selects the tuple quad).
        const int sa = lh ? 116 : 127, sb = lh ? 129 : 118;
        h8 ah0[MB], ah1[MB], ah2[MB], bh0[NBW], bh1[NBW], bh2[NBW];
        i32x8 al01[MB], bl01[NBW], al2[MB], bl2[NBW];
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) { ah2[mb] = h8{}; al2[mb] = i32x8{}; al01[mb] = i32x8{}; }
#pragma unroll
        for (int nb = 0; nb < NBW; ++nb) { bh2[nb] = h8{}; bl2[nb] = i32x8{}; bl01[nb] = i32x8{}; }
        constexpr int NM = MB * NBW, NF = MB + NBW;       // MFMAs per group; fragment reads per (tap, hi or lo)
        // one fragment read: index i < MB: weights of block i, else activations of pixel row i - MB; hl = 0 hi, 1 lo
        auto rd_hi = [&](auto i_, h8 (&a)[MB], h8 (&b)[NBW], const h8* wb, const h8* xb, int ky, int kx) {
            constexpr int i = decltype(i_)::value;
            if constexpr (i < MB) a[i] = wb[a_base + kx * 4 * CO_WG + i * 32];
            else b[i - MB] = xb[b_base + (i - MB + ky) * TWP + kx];
        };
        auto rd_lo = [&](auto i_, auto q_, i32x8 (&a)[MB], i32x8 (&b)[NBW], const h8* wb, const h8* xb, int ky, int kx) {
            constexpr int i = decltype(i_)::value, q = decltype(q_)::value;
            if constexpr (i < MB) { NB_Q(a[i], q, wb[a_base + kx * 4 * CO_WG + CO_WG + i * 32]); }
            else { NB_Q(b[i - MB], q, xb[b_base + XPL + (i - MB + ky) * TWP + kx]); }
        };
        // a group of NM MFMAs (tile k = (k / NBW, k % NBW)) with NFILL fillers dealt evenly into the gaps behind them
        auto group = [&](auto nfill_, auto&& mf, auto&& ff) {
            constexpr int NFILL = decltype(nfill_)::value;
            nb_static_for<0, NM>([&](auto k_) {
                constexpr int k = decltype(k_)::value;
                mf(std::integral_constant<int, k / NBW>{}, std::integral_constant<int, k % NBW>{});
                NB_SB;
                nb_static_for<0, NFILL>([&](auto i_) {
                    constexpr int i = decltype(i_)::value;
                    if constexpr (i * NM / (NFILL > 0 ? NFILL : 1) == k) ff(i_);
                });
                NB_SB;
            });
        };
        // (q: which half of the accumulator tile the NB_MOCK16 timing build writes; unused otherwise)
        auto mf_f16 = [&](h8 (&a)[MB], h8 (&b)[NBW], int q = 0) {
            return [&, q](auto mb_, auto nb_) {
                constexpr int mb = decltype(mb_)::value, nb = decltype(nb_)::value;
                acc[mb][nb] = NB_MFMA_F16(a[mb], b[nb], acc[mb][nb], q);
            };
        };
        auto mf_fp8 = [&](i32x8 (&a)[MB], i32x8 (&b)[NBW], int q = 0) {
            return [&, q](auto mb_, auto nb_) {
                constexpr int mb = decltype(mb_)::value, nb = decltype(nb_)::value;
                if constexpr (!HO) acc[mb][nb] = NB_MFMA_FP8(a[mb], b[nb], acc[mb][nb], sa, sb, q);
            };
        };
        using K0 = std::integral_constant<int, 0>; using K1 = std::integral_constant<int, 1>; using K2 = std::integral_constant<int, 2>;
        if constexpr (PPK) {
            // ---- ping-pong: LOAD(t) = the pieces of sub-chunk t + 3 (on KY = 0 also the next chunk's halo tile), then every fragment of
            //      step t; COMPUTE(t) = tap 0, tap 1, corrections 0 + 1, tap 2, on odd t the tap-2 corrections of steps t-1 and t.
            //   segment      0        1        2        3        4
            //   waves 0-3   LOAD 0   COMP 0   LOAD 1   COMP 1   LOAD 2  ...        (one barrier after every segment)
            //   waves 4-7   (wait)   LOAD 0   COMP 0   LOAD 1   COMP 1  ...
            // Stage t (weight ring slot t & 3, halo tile of its chunk) is read in segments 2t (waves 0-3) and 2t + 1 (waves 4-7); the
            // barrier that ends segment 2t + 1 is the one in front of which every wave waits for its pieces up to sub-chunk t + 1
            // (all but the youngest two sub-chunks, + the halo tile unless it is due), so stage t + 1 has landed when segment 2t + 2
            // starts to read it, and slot (t + 3) & 3 = (t - 1) & 3, which LOAD(t) refills, was last read in segment 2t - 1.
            auto load_seg = [&](auto ky_, auto odd_, int t, int c) {
                constexpr int KY = decltype(ky_)::value, ODD = decltype(odd_)::value;
                const h8* xb = xbuf + (c & 1) * 4 * XPL;
                const h8* wb = wring + (t & 3) * WSLOTS;
                NB_SB;
                nb_static_for<0, NF>([&](auto i_) { rd_hi(i_, ah0, bh0, wb, xb, KY, 0); });
                nb_static_for<0, NF>([&](auto i_) { rd_hi(i_, ah1, bh1, wb, xb, KY, 1); });
                nb_static_for<0, NF>([&](auto i_) { rd_lo(i_, std::integral_constant<int, 0>{}, al01, bl01, wb, xb, KY, 0); });
                nb_static_for<0, NF>([&](auto i_) { rd_lo(i_, std::integral_constant<int, 1>{}, al01, bl01, wb, xb, KY, 1); });
                nb_static_for<0, NF>([&](auto i_) { rd_hi(i_, ah2, bh2, wb, xb, KY, 2); });
                nb_static_for<0, NF>([&](auto i_) { rd_lo(i_, std::integral_constant<int, ODD>{}, al2, bl2, wb, xb, KY, 2); });
                NB_SB;
            };
            // COMPUTE(t): the step's MFMAs; its LDS-DMA pieces (sub-chunk t + 3, on KY = 0 the next chunk's halo tile) ride in the gaps
            // behind the first two groups (slot (t + 3) & 3 was last read in segment 2t - 1; this is segment 2t + 1 or 2t + 2)
            auto comp_seg = [&](auto ky_, auto odd_, int t, int c) {
                constexpr int KY = decltype(ky_)::value, ODD = decltype(odd_)::value;
                constexpr int NDMA = NWPW + (KY == 0 ? NXPW : 0);
                const int t3 = clampt(t + 3), c1 = c + 1 < NC ? c + 1 : NC - 1;
                auto dma = [&](auto i_) {
                    constexpr int i = decltype(i_)::value;
                    if constexpr (i < NWPW) issue_w_v2(i_, t3, (t + 3) & 3);
                    else issue_x_v2(std::integral_constant<int, i - NWPW>{}, c1, (c + 1) & 1);
                };
                NB_SB;
                // (a piece costs the wave ~60 cycles of issue: behind a 64-cycle fp8 MFMA it is hidden, behind a 32-cycle f16 one the pipe waits)
                constexpr int N1 = NDMA < NM ? NDMA : NM, R = NDMA - N1;
                auto dma_r = [&](auto i_) { dma(std::integral_constant<int, decltype(i_)::value + N1>{}); };
                group(std::integral_constant<int, 0>{}, mf_f16(ah0, bh0, 0), [](auto) {});
                group(std::integral_constant<int, 0>{}, mf_f16(ah1, bh1, 1), [](auto) {});
                group(std::integral_constant<int, N1>{}, mf_fp8(al01, bl01, 0), dma);
                group(std::integral_constant<int, ODD ? 0 : R>{}, mf_f16(ah2, bh2, 1), dma_r);
                if constexpr (ODD) group(std::integral_constant<int, R>{}, mf_fp8(al2, bl2, 0), dma_r);
                NB_SB;
            };
            const bool grp_b = wv >= 4;
            // one step of a wave: LOAD, sync, COMPUTE, sync.  The counted vmcnt wait stands in front of the barrier that ends an ODD
            // segment -- behind COMPUTE(t) for waves 0-3 (pieces up to sub-chunk t + 3 issued: the youngest two sub-chunks may be in flight,
            // and the halo tile unless it is due), behind LOAD(t) for waves 4-7 (issued up to t + 2: the youngest one).
            auto pp_step = [&](auto b_, auto ky_, auto odd_, int t, int c) {
                constexpr bool B = decltype(b_)::value;
                constexpr int KY = decltype(ky_)::value;
                constexpr int NVA = KY == 2 ? 2 * NWPW : 2 * NWPW + NXPW, NVB = KY == 1 ? NWPW + NXPW : NWPW;
#ifdef NB_PP_STAMPS
                const unsigned long long s0 = __builtin_amdgcn_s_memtime();
#endif
                load_seg(ky_, odd_, t, c);
#ifdef NB_PP_STAMPS
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                const unsigned long long s1 = __builtin_amdgcn_s_memtime();
#endif
                if constexpr (B) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(NVB) : "memory");
                else asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
#ifdef NB_PP_STAMPS
                const unsigned long long s2 = __builtin_amdgcn_s_memtime();
#endif
                comp_seg(ky_, odd_, t, c);
#ifdef NB_PP_STAMPS
                const unsigned long long s3 = __builtin_amdgcn_s_memtime();
#endif
                if constexpr (B) asm volatile("s_barrier" ::: "memory");
                else asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(NVA) : "memory");
#ifdef NB_PP_STAMPS
                const unsigned long long s4 = __builtin_amdgcn_s_memtime();
                t_dma += ((s1 - s0) & 0xffffffffull) | ((s3 - s2) << 32);          // (load | compute) cycles
                t_bar += ((s2 - s1) & 0xffffffffull) | ((s4 - s3) << 32);          // (wait behind load | wait behind compute)
#endif
            };
            auto pp_loop = [&](auto b_) {
                int c = 0;
                for (; c + 1 < NC; c += 2) {
                    pp_step(b_, K0{}, K0{}, 3 * c, c); pp_step(b_, K1{}, K1{}, 3 * c + 1, c); pp_step(b_, K2{}, K0{}, 3 * c + 2, c);
                    pp_step(b_, K0{}, K1{}, 3 * c + 3, c + 1); pp_step(b_, K1{}, K0{}, 3 * c + 4, c + 1); pp_step(b_, K2{}, K1{}, 3 * c + 5, c + 1);
                }
                if (c < NC) { pp_step(b_, K0{}, K0{}, 3 * c, c); pp_step(b_, K1{}, K1{}, 3 * c + 1, c); pp_step(b_, K2{}, K0{}, 3 * c + 2, c); }
            };
            if (grp_b) {
                asm volatile("s_barrier" ::: "memory");
                pp_loop(std::true_type{});
            } else {
                pp_loop(std::false_type{});
                asm volatile("s_barrier" ::: "memory");
            }
            NB_SB;
            if (T & 1) {                                   // an odd number of steps: the last tuple of tap-2 corrections holds one tap only
#pragma unroll
                for (int mb = 0; mb < MB; ++mb)
#pragma unroll
                    for (int r = 4; r < 8; ++r) al2[mb][r] = 0;
#pragma unroll
                for (int nb = 0; nb < NBW; ++nb)
#pragma unroll
                    for (int r = 4; r < 8; ++r) bl2[nb][r] = 0;
                group(std::integral_constant<int, 0>{}, mf_fp8(al2, bl2), [](auto) {});
            }
        } else {
        // step t: KY = tap row, ODD = t & 1 (compile time); reads stage (c, slot t & 3), issues sub-chunk t + 3 (and on KY = 0 the
        // next chunk's halo tile), pre-reads step t + 1
        auto step = [&](auto ky_, auto odd_, int t, int c) {
            constexpr int KY = decltype(ky_)::value, ODD = decltype(odd_)::value;
            constexpr int NDMA = NWPW + (KY == 0 ? NXPW : 0);
            const h8* xb = xbuf + (c & 1) * 4 * XPL;
            const h8* wb = wring + (t & 3) * WSLOTS;
            const int tn = t + 1, cn = KY == 2 ? c + 1 : c;
            constexpr int KYN = KY == 2 ? 0 : KY + 1;
            const h8* xbn = xbuf + (cn & 1) * 4 * XPL;
            const h8* wbn = wring + (tn & 3) * WSLOTS;
            const int t3 = clampt(t + 3), c1 = c + 1 < NC ? c + 1 : NC - 1;
            auto dma = [&](auto i_) {
                constexpr int i = decltype(i_)::value;
                if constexpr (i < NWPW) issue_w_v2(i_, t3, (t + 3) & 3);
                else issue_x_v2(std::integral_constant<int, i - NWPW>{}, c1, (c + 1) & 1);
            };
            NB_SB;
            // part A
            group(std::integral_constant<int, NDMA>{}, mf_f16(ah2, bh2), dma);                       // tap 2 of step t-1
            if constexpr (!ODD) {
                group(std::integral_constant<int, NF>{}, mf_fp8(al2, bl2),                            // tap-2 corrections of t-2, t-1
                      [&](auto i_) { rd_hi(i_, ah2, bh2, wb, xb, KY, 2); });
                group(std::integral_constant<int, NF>{}, mf_f16(ah0, bh0),                            // tap 0
                      [&](auto i_) { rd_lo(i_, std::integral_constant<int, 0>{}, al2, bl2, wb, xb, KY, 2); });
            } else {
                group(std::integral_constant<int, 2 * NF>{}, mf_f16(ah0, bh0), [&](auto i_) {         // tap 0
                    constexpr int i = decltype(i_)::value;
                    if constexpr (i < NF) rd_hi(i_, ah2, bh2, wb, xb, KY, 2);
                    else rd_lo(std::integral_constant<int, i - NF>{}, std::integral_constant<int, 1>{}, al2, bl2, wb, xb, KY, 2);
                });
            }
            // everything issued before sub-chunk t-1 has landed (it is what step t+1 reads); all reads of stage t are done
            if constexpr (KY == 2) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(2 * NWPW) : "memory");
            else asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(2 * NWPW + NXPW) : "memory");
            NB_SB;
            // part B
            group(std::integral_constant<int, NF>{}, mf_f16(ah1, bh1),                                // tap 1
                  [&](auto i_) { rd_hi(i_, ah0, bh0, wbn, xbn, KYN, 0); });
            group(std::integral_constant<int, NF>{}, mf_fp8(al01, bl01),                              // corrections of taps 0 + 1
                  [&](auto i_) { rd_hi(i_, ah1, bh1, wbn, xbn, KYN, 1); });
            nb_static_for<0, NF>([&](auto i_) { rd_lo(i_, std::integral_constant<int, 0>{}, al01, bl01, wbn, xbn, KYN, 0); });
            nb_static_for<0, NF>([&](auto i_) { rd_lo(i_, std::integral_constant<int, 1>{}, al01, bl01, wbn, xbn, KYN, 1); });
            NB_SB;
        };
        // operands of step 0
        nb_static_for<0, NF>([&](auto i_) { rd_hi(i_, ah0, bh0, wring, xbuf, 0, 0); });
        nb_static_for<0, NF>([&](auto i_) { rd_hi(i_, ah1, bh1, wring, xbuf, 0, 1); });
        nb_static_for<0, NF>([&](auto i_) { rd_lo(i_, std::integral_constant<int, 0>{}, al01, bl01, wring, xbuf, 0, 0); });
        nb_static_for<0, NF>([&](auto i_) { rd_lo(i_, std::integral_constant<int, 1>{}, al01, bl01, wring, xbuf, 0, 1); });
        int c = 0;
        for (; c + 1 < NC; c += 2) {                   // t = 3 c is even here
            step(K0{}, K0{}, 3 * c, c); step(K1{}, K1{}, 3 * c + 1, c); step(K2{}, K0{}, 3 * c + 2, c);
            step(K0{}, K1{}, 3 * c + 3, c + 1); step(K1{}, K0{}, 3 * c + 4, c + 1); step(K2{}, K1{}, 3 * c + 5, c + 1);
        }
        if (c < NC) { step(K0{}, K0{}, 3 * c, c); step(K1{}, K1{}, 3 * c + 1, c); step(K2{}, K0{}, 3 * c + 2, c); }
        NB_SB;
        // the last step's tap 2 and the last tuple of tap-2 corrections (an odd number of steps: it holds one tap only)
        nb_static_for<0, NM>([&](auto k_) { constexpr int k = decltype(k_)::value; mf_f16(ah2, bh2)(std::integral_constant<int, k / NBW>{}, std::integral_constant<int, k % NBW>{}); NB_SB; });
        if (T & 1) {
#pragma unroll
            for (int mb = 0; mb < MB; ++mb)
#pragma unroll
                for (int r = 4; r < 8; ++r) al2[mb][r] = 0;
#pragma unroll
            for (int nb = 0; nb < NBW; ++nb)
#pragma unroll
                for (int r = 4; r < 8; ++r) bl2[nb][r] = 0;
        }
        nb_static_for<0, NM>([&](auto k_) { constexpr int k = decltype(k_)::value; mf_fp8(al2, bl2)(std::integral_constant<int, k / NBW>{}, std::integral_constant<int, k % NBW>{}); NB_SB; });
        }
    } else if constexpr (V2) {
        // ---- H2 operands (the `h3` arithmetic: hi x hi, hi x lo, lo x hi per tap), software-pipelined over the barrier like the
        //      f8 loop above.  Per accumulator tile the nine products of a step arrive in the order of the loop below (tap by tap:
        //      hh, hl, lh): bit-identical.  Step t:
        //   part A:  taps 0 and 1 (six groups of four MFMAs: one product kind of one tap over the four tiles -- no two MFMAs in a row on
        //            one accumulator)            fillers: the step's LDS-DMA pieces, its tap-2 fragments
        //   wait (counted) + barrier: every wave has read ALL of stage t; stage t+1 has landed
        //   part B:  tap 2 (three groups)         fillers: the sixteen fragments of taps 0 and 1 of step t+1
        h8 ah[3][MB], al[3][MB], bh[3][NBW], bl[3][NBW];           // [tap][block]
#pragma unroll
        for (int k = 0; k < 3; ++k) {
#pragma unroll
            for (int mb = 0; mb < MB; ++mb) { ah[k][mb] = h8{}; al[k][mb] = h8{}; }
#pragma unroll
            for (int nb = 0; nb < NBW; ++nb) { bh[k][nb] = h8{}; bl[k][nb] = h8{}; }
        }
        constexpr int NM = MB * NBW, NF = MB + NBW;
        // fragment read j of a tap (0 .. 2 NF - 1): hi fragments (weights of block i, then activations of pixel row i - MB), then lo
        auto rd = [&](auto j_, auto kx_, const h8* wb, const h8* xb, int ky) {
            constexpr int j = decltype(j_)::value, kx = decltype(kx_)::value, hl = j / NF, i = j % NF;
            if constexpr (i < MB) (hl ? al : ah)[kx][i] = wb[a_base + kx * 4 * CO_WG + hl * CO_WG + i * 32];
            else (hl ? bl : bh)[kx][i - MB] = xb[b_base + hl * XPL + (i - MB + ky) * TWP + kx];
        };
        // group g of NG: NM MFMAs of one product kind with the fillers [g L / NG, (g + 1) L / NG) of a list of L dealt into its gaps
        auto group = [&](auto g_, auto ng_, auto l_, auto&& mf, auto&& item) {
            constexpr int g = decltype(g_)::value, NG = decltype(ng_)::value, L = decltype(l_)::value;
            constexpr int lo = g * L / NG, hi = (g + 1) * L / NG, NFILL = hi - lo;
            nb_static_for<0, NM>([&](auto k_) {
                constexpr int k = decltype(k_)::value;
                mf(std::integral_constant<int, k / NBW>{}, std::integral_constant<int, k % NBW>{});
                NB_SB;
                nb_static_for<0, NFILL>([&](auto i_) {
                    constexpr int i = decltype(i_)::value;
                    if constexpr (i * NM / (NFILL > 0 ? NFILL : 1) == k) item(std::integral_constant<int, lo + i>{});
                });
                NB_SB;
            });
        };
        // product kind q of tap kx: 0 = hi x hi, 1 = hi x lo, 2 = lo x hi
        auto mf = [&](auto kx_, auto q_) {
            return [&](auto mb_, auto nb_) {
                constexpr int kx = decltype(kx_)::value, q = decltype(q_)::value, mb = decltype(mb_)::value, nb = decltype(nb_)::value;
                acc[mb][nb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(q == 2 ? al[kx][mb] : ah[kx][mb], q == 1 ? bl[kx][nb] : bh[kx][nb], acc[mb][nb], 0, 0, 0);
            };
        };
        using I0 = std::integral_constant<int, 0>; using I1 = std::integral_constant<int, 1>; using I2 = std::integral_constant<int, 2>;
        using I3 = std::integral_constant<int, 3>; using I4 = std::integral_constant<int, 4>; using I5 = std::integral_constant<int, 5>;
        using I6 = std::integral_constant<int, 6>;
        auto step = [&](auto ky_, int t, int c) {
            constexpr int KY = decltype(ky_)::value;
            constexpr int NDMA = NWPW + (KY == 0 ? NXPW : 0);
            const h8* xb = xbuf + (c & 1) * 4 * XPL;
            const h8* wb = wring + (t & 3) * WSLOTS;
            const int tn = t + 1, cn = KY == 2 ? c + 1 : c;
            constexpr int KYN = KY == 2 ? 0 : KY + 1;
            const h8* xbn = xbuf + (cn & 1) * 4 * XPL;
            const h8* wbn = wring + (tn & 3) * WSLOTS;
            const int t3 = clampt(t + 3), c1 = c + 1 < NC ? c + 1 : NC - 1;
            // part A's fillers: the pieces, then this step's tap-2 fragments
            using LA = std::integral_constant<int, NDMA + 2 * NF>;
            auto item_a = [&](auto i_) {
                constexpr int i = decltype(i_)::value;
                if constexpr (i < NWPW) issue_w_v2(i_, t3, (t + 3) & 3);
                else if constexpr (i < NDMA) issue_x_v2(std::integral_constant<int, i - NWPW>{}, c1, (c + 1) & 1);
                else rd(std::integral_constant<int, i - NDMA>{}, I2{}, wb, xb, KY);
            };
            // part B's: taps 0 and 1 of step t + 1
            using LB = std::integral_constant<int, 4 * NF>;
            auto item_b = [&](auto i_) {
                constexpr int i = decltype(i_)::value;
                if constexpr (i < 2 * NF) rd(i_, I0{}, wbn, xbn, KYN);
                else rd(std::integral_constant<int, i - 2 * NF>{}, I1{}, wbn, xbn, KYN);
            };
            NB_SB;
            group(I0{}, I6{}, LA{}, mf(I0{}, I0{}), item_a); group(I1{}, I6{}, LA{}, mf(I0{}, I1{}), item_a); group(I2{}, I6{}, LA{}, mf(I0{}, I2{}), item_a);
            group(I3{}, I6{}, LA{}, mf(I1{}, I0{}), item_a); group(I4{}, I6{}, LA{}, mf(I1{}, I1{}), item_a); group(I5{}, I6{}, LA{}, mf(I1{}, I2{}), item_a);
            // everything issued before sub-chunk t-1 has landed (it is what step t+1 reads); all reads of stage t are done
            if constexpr (KY == 2) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(2 * NWPW) : "memory");
            else asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(2 * NWPW + NXPW) : "memory");
            NB_SB;
            group(I0{}, I3{}, LB{}, mf(I2{}, I0{}), item_b); group(I1{}, I3{}, LB{}, mf(I2{}, I1{}), item_b); group(I2{}, I3{}, LB{}, mf(I2{}, I2{}), item_b);
            NB_SB;
        };
        // operands of step 0
        nb_static_for<0, 2 * NF>([&](auto j_) { rd(j_, I0{}, wring, xbuf, 0); });
        nb_static_for<0, 2 * NF>([&](auto j_) { rd(j_, I1{}, wring, xbuf, 0); });
        for (int c = 0; c < NC; ++c) { step(I0{}, 3 * c, c); step(I1{}, 3 * c + 1, c); step(I2{}, 3 * c + 2, c); }
        NB_SB;
    } else if constexpr (F8) {
        // ---- f8 operands: explicitly ordered, software-pipelined step -------------------------------------------
        // The compiler, left alone, sinks every fragment read to just before its first use and waits with lgkmcnt(0)
        // right after issuing it (five exposed LDS latencies per step with both waves of a SIMD in lockstep).  Here
        // every statement group is followed by a scheduling fence, so the program order below is the issue order:
        //     after barrier(t-1):  reads tap 0, tap 1 of step t | tap 2 main of step t-1 (4 x 32 cycles of cover) |
        //                          on even t: tap-2 corrections of steps t-2 and t-1 together (4 x 64 cycles)
        //     tap 0 main | reads tap 2 | tap 1 main | corrections taps 0+1 | DMA issues | wait | barrier(t)
        // i.e. a fragment is read at least one matrix group (128-256 cycles) before the group that consumes it.
        // The third tap of a row has no partner within its step, so its corrections ride with the third tap of the NEXT step
        // in one K = 64 fp8 instruction (quad 0 = even step, quad 1 = odd step): 7 fp8 instructions per two steps instead of
        // 8, 768 instead of 896 matrix cycles per step and tile row.
        const int sa = lh ? 116 : 127, sb = lh ? 129 : 118;
        h8 ah0[MB], ah1[MB], ah2[MB], bh0[NBW], bh1[NBW], bh2[NBW];
        i32x8 al01[MB], bl01[NBW], al2[MB], bl2[NBW];          // fp8 operand tuples: (tap 0 | tap 1), (tap 2 of an even step | of the odd step after it)
#pragma unroll
        for (int mb = 0; mb < MB; ++mb)
#pragma unroll
            for (int r = 0; r < 8; ++r) al2[mb][r] = 0;
#pragma unroll
        for (int nb = 0; nb < NBW; ++nb)
#pragma unroll
            for (int r = 0; r < 8; ++r) bl2[nb][r] = 0;
        auto rd_tap01 = [&](const h8* wb, const h8* xb, int ky, int kx) {       // kx = 0 or 1: hi fragments + quad kx of the lo tuples
#pragma unroll
            for (int mb = 0; mb < MB; ++mb) {
                (kx ? ah1 : ah0)[mb] = wb[a_base + kx * 4 * CO_WG + mb * 32];
                if (kx) { NB_Q(al01[mb], 1, wb[a_base + kx * 4 * CO_WG + CO_WG + mb * 32]); } else { NB_Q(al01[mb], 0, wb[a_base + CO_WG + mb * 32]); }
            }
#pragma unroll
            for (int nb = 0; nb < NBW; ++nb) {
                (kx ? bh1 : bh0)[nb] = xb[b_base + (nb + ky) * TWP + kx];
                if (kx) { NB_Q(bl01[nb], 1, xb[b_base + XPL + (nb + ky) * TWP + kx]); } else { NB_Q(bl01[nb], 0, xb[b_base + XPL + (nb + ky) * TWP]); }
            }
            NB_SB;
        };
        auto rd_tap2 = [&](const h8* wb, const h8* xb, int ky, int odd) {       // odd = quad of the tap-2 tuples
#pragma unroll
            for (int mb = 0; mb < MB; ++mb) {
                ah2[mb] = wb[a_base + 2 * 4 * CO_WG + mb * 32];
                if (odd) { NB_Q(al2[mb], 1, wb[a_base + 2 * 4 * CO_WG + CO_WG + mb * 32]); } else { NB_Q(al2[mb], 0, wb[a_base + 2 * 4 * CO_WG + CO_WG + mb * 32]); }
            }
#pragma unroll
            for (int nb = 0; nb < NBW; ++nb) {
                bh2[nb] = xb[b_base + (nb + ky) * TWP + 2];
                if (odd) { NB_Q(bl2[nb], 1, xb[b_base + XPL + (nb + ky) * TWP + 2]); } else { NB_Q(bl2[nb], 0, xb[b_base + XPL + (nb + ky) * TWP + 2]); }
            }
            NB_SB;
        };
        auto main4 = [&](h8 (&a)[MB], h8 (&b)[NBW]) {
#pragma unroll
            for (int mb = 0; mb < MB; ++mb)
#pragma unroll
                for (int nb = 0; nb < NBW; ++nb) { acc[mb][nb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[mb], b[nb], acc[mb][nb], 0, 0, 0); NB_SB; }
        };
        auto corr4 = [&](i32x8 (&a)[MB], i32x8 (&b)[NBW]) {
#pragma unroll
            for (int mb = 0; mb < MB; ++mb)
#pragma unroll
                for (int nb = 0; nb < NBW; ++nb) {
                    acc[mb][nb] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a[mb], b[nb], acc[mb][nb], 0, 0, 0, sa, 0, sb);
                    NB_SB;
                }
        };
        // the loop runs over PAIRS of steps (t = 2 tp, 2 tp + 1) so that the tuple quad is a compile-time constant
        auto step = [&](int t, int odd, bool first) {
            const int c = t / 3, ky = t - 3 * c;
            const h8* xb = xbuf + (c & 1) * 4 * XPL;
            const h8* wb = wring + (t & 3) * WSLOTS;
            NB_SB;
            rd_tap01(wb, xb, ky, 0);
            rd_tap01(wb, xb, ky, 1);
            if (!first) main4(ah2, bh2);               // tap 2 of the previous step
            if (!odd && !first) corr4(al2, bl2);       // tap-2 corrections of the two previous steps
            main4(ah0, bh0);
            rd_tap2(wb, xb, ky, odd);
            main4(ah1, bh1);
            corr4(al01, bl01);
            // keep the LDS-DMA stream 3 sub-chunks ahead (past the end: harmless re-copies keep the counts uniform)
            issue_w(clampt(t + 3), wring + ((t + 3) & 3) * WSLOTS);
            if (ky == 0) issue_x(c + 1 < NC ? c + 1 : NC - 1, xbuf + ((c + 1) & 1) * 4 * XPL);
            NB_SB;
            // everything issued before sub-chunk t-1 must have landed (it is what sub-chunk t+1 reads)
            if (ky == 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * NWPW) : "memory");
            else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * NWPW + NXPW) : "memory");
            __builtin_amdgcn_s_barrier();
        };
        for (int t = 0; t < T; t += 2) {
            step(t, 0, t == 0);
            if (t + 1 < T) step(t + 1, 1, false);
        }
        NB_SB;
        main4(ah2, bh2);                               // the last step's tap 2
        if (T & 1) {                                   // odd number of steps: the last tuple holds one tap only
#pragma unroll
            for (int mb = 0; mb < MB; ++mb)
#pragma unroll
                for (int r = 4; r < 8; ++r) al2[mb][r] = 0;
#pragma unroll
            for (int nb = 0; nb < NBW; ++nb)
#pragma unroll
                for (int r = 4; r < 8; ++r) bl2[nb][r] = 0;
        }
        corr4(al2, bl2);
#undef NB_Q
#undef NB_SB
    } else
    for (int c = 0; c < NC; ++c) {
        const h8* xb = xbuf + (c & 1) * 4 * XPL;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const int t = c * 3 + ky;
            // keep the LDS-DMA stream 3 sub-chunks ahead (past the end: harmless re-copies keep the counts uniform)
            if (!(p.dbg & 2)) {
                issue_w(clampt(t + 3), wring + ((t + 3) & 3) * WSLOTS);
                if (ky == 0) issue_x(c + 1 < NC ? c + 1 : NC - 1, xbuf + ((c + 1) & 1) * 4 * XPL);
            }
            __builtin_amdgcn_sched_barrier(0);
            const h8* wb = wring + (t & 3) * WSLOTS;
            h8 ah[2][MB], al[2][MB], bh[2][NBW], bl[2][NBW];
            auto fetch = [&](int kx, h8 (&fah)[MB], h8 (&fal)[MB], h8 (&fbh)[NBW], h8 (&fbl)[NBW]) {
#pragma unroll
                for (int mb = 0; mb < MB; ++mb) {
                    fah[mb] = wb[a_base + kx * 4 * CO_WG + mb * 32];
                    fal[mb] = wb[a_base + kx * 4 * CO_WG + CO_WG + mb * 32];
                }
#pragma unroll
                for (int nb = 0; nb < NBW; ++nb) {
                    fbh[nb] = xb[b_base + (nb + ky) * TWP + kx];
                    fbl[nb] = xb[b_base + XPL + (nb + ky) * TWP + kx];
                }
            };
            fetch(0, ah[0], al[0], bh[0], bl[0]);
            if (F8) {
                // block scales (E8M0) of this lane's 32-element K block: lh = 0 -> fp8(w) * fp8(xl 2^9), lh = 1 -> fp8(wl 2^11) * fp8(x/4)
                const int sa = lh ? 116 : 127, sb = lh ? 129 : 118;
                const h8 z8 = {};
                // tap 0: main products; tap 1's fragments arrive meanwhile
#pragma unroll
                for (int mb = 0; mb < MB; ++mb)
#pragma unroll
                    for (int nb = 0; nb < NBW; ++nb) {
                        acc[mb][nb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[0][mb], bh[0][nb], acc[mb][nb], 0, 0, 0);
                        if (mb + nb == 0) fetch(1, ah[1], al[1], bh[1], bl[1]);
                    }
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x100, 2 * MB + 2 * NBW, 0);
                __builtin_amdgcn_sched_group_barrier(0x008, MB * NBW - 1, 0);
                // taps 0+1: corrections (one fp8 MFMA per tile), then tap 1's main products; tap 2's fragments replace tap 0's
#pragma unroll
                for (int mb = 0; mb < MB; ++mb)
#pragma unroll
                    for (int nb = 0; nb < NBW; ++nb)
                        acc[mb][nb] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(nb_cat8(al[0][mb], al[1][mb]), nb_cat8(bl[0][nb], bl[1][nb]),
                                                                                      acc[mb][nb], 0, 0, 0, sa, 0, sb);
                fetch(2, ah[0], al[0], bh[0], bl[0]);
#pragma unroll
                for (int mb = 0; mb < MB; ++mb)
#pragma unroll
                    for (int nb = 0; nb < NBW; ++nb)
                        acc[mb][nb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[1][mb], bh[1][nb], acc[mb][nb], 0, 0, 0);
                __builtin_amdgcn_sched_group_barrier(0x008, MB * NBW, 0);
                __builtin_amdgcn_sched_group_barrier(0x100, 2 * MB + 2 * NBW, 0);
                __builtin_amdgcn_sched_group_barrier(0x008, MB * NBW, 0);
                // tap 2: main products and its corrections (second half of the fp8 K block empty)
#pragma unroll
                for (int mb = 0; mb < MB; ++mb)
#pragma unroll
                    for (int nb = 0; nb < NBW; ++nb) {
                        acc[mb][nb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[0][mb], bh[0][nb], acc[mb][nb], 0, 0, 0);
                        acc[mb][nb] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(nb_cat8(al[0][mb], z8), nb_cat8(bl[0][nb], z8),
                                                                                      acc[mb][nb], 0, 0, 0, sa, 0, sb);
                    }
            } else {
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int cu = kx & 1;
                acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[cu][0], bh[cu][0], acc[0][0], 0, 0, 0);
                if (kx + 1 < 3) fetch(kx + 1, ah[cu ^ 1], al[cu ^ 1], bh[cu ^ 1], bl[cu ^ 1]);
#pragma unroll
                for (int mb = 0; mb < MB; ++mb)
#pragma unroll
                    for (int nb = 0; nb < NBW; ++nb) {
                        if (mb + nb > 0)
                            acc[mb][nb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[cu][mb], bh[cu][nb], acc[mb][nb], 0, 0, 0);
                        acc[mb][nb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[cu][mb], bl[cu][nb], acc[mb][nb], 0, 0, 0);
                        acc[mb][nb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[cu][mb], bh[cu][nb], acc[mb][nb], 0, 0, 0);
                    }
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                if (kx + 1 < 3) __builtin_amdgcn_sched_group_barrier(0x100, 2 * MB + 2 * NBW, 0);
                __builtin_amdgcn_sched_group_barrier(0x008, 3 * MB * NBW - 1, 0);
            }
            }
            __builtin_amdgcn_sched_barrier(0);
            unsigned long long tw0 = 0;
            if (p.tstamps) tw0 = __builtin_amdgcn_s_memtime();
            // everything issued before sub-chunk t-1 must have landed (it is what sub-chunk t+1 reads)
            if (ky == 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * NWPW) : "memory");
            else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * NWPW + NXPW) : "memory");
            if (p.tstamps) { const unsigned long long tw1 = __builtin_amdgcn_s_memtime(); t_dma += tw1 - tw0; tw0 = tw1; }
            __builtin_amdgcn_s_barrier();
            if (p.tstamps) t_bar += __builtin_amdgcn_s_memtime() - tw0;
        }
    }
#ifdef NB_PP_STAMPS
    if (p.tstamps && tid == 0) {
        unsigned long long* ts = p.tstamps + (size_t)item * 8;
        ts[6] = t_dma; ts[7] = t_bar;
    }
#else
    if (p.tstamps && tid == 0) {
        unsigned it_ = item; asm volatile("" : "+v"(it_));
        unsigned long long* ts = p.tstamps + (size_t)it_ * 8;
        ts[6] = t_dma; ts[7] = t_bar | ((__builtin_amdgcn_s_memtime() - t_loop0) << 32);
    }
#endif
    // drain the tail re-copies before the staging LDS is reused: every wave waits for ITS pieces, and the barrier makes
    // sure no other wave's late piece lands on top of epilogue data (without it the outcome depended on DMA timing)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    NB_TSTAMP(2);
    if (p.dbg & 4) { if (acc[0][0][0] == 123.456f) p.y[0] = 0.f; return; }      // ablation: main loop only
    // ---- the NEXT tile's prologue goes out now, ahead of this tile's epilogue, where that epilogue works straight from the accumulators
    //      (hand-off output; the fused ToRGB of a 64-channel layer): its ~4 us of LDS-DMA round trip then pass under the epilogue's
    //      arithmetic and stores.  The fp32-output path stages its tile in the LDS the prologue fills: there the prologue follows it.
    //      The epilogue keeps THIS tile's coordinates (e_*). ----
    const int e_n = n, e_y0 = y0, e_x0 = x0, e_co0 = co0;
    const unsigned item_next = PERSIST ? __builtin_amdgcn_readfirstlane(item + gridDim.x) : total;
    const bool lds_free_epilogue = p.yh2 || (MW == 1 && p.tg.c && !p.y && p.c_out % 8 == 0);
    const bool early = item_next < total && lds_free_epilogue && !(p.dbg & 64);      // (dbg & 64: no prefetch)
    if (item_next < total) {
        tile_coords(item_next);
        piece_offsets();
        if constexpr (V2) piece_sources_v2();
        if (early) prologue_issue();
    }
    auto epilogue = [&]() {

    // ---- epilogue: *d, +noise, +bias, lrelu, gain, clamp -> fp32 NCHW; D[row = c_out, col = pixel] ----
    // The finished values go through LDS (the staging buffers are dead now) as an [c_out][pixel] image so that each
    // lane can store 16 bytes (4 consecutive pixels of one channel row): 4x fewer store instructions than storing
    // the accumulator registers directly, and whole 512-byte row segments per wave-instruction.
    constexpr int PIX_WG = TH * 32;
    if (p.yh2) {
        // (the gain through a vector register of its own: see gain_t below)
        float gain_h = p.gain;
        asm volatile("" : "+v"(gain_h));
        const H3HandoffArgs ha_ = nb_handoff_args(p.yh2, p.c8_next, p.c_out, p.h, p.w, p.out_f8, p.dbg, p.alpha, gain_h, p.clamp);
        if constexpr (F8 && V2) {          // (the f6 output form exists for the software-pipelined f8 / f6 kernels only: the launcher checks)
            if (p.out_f8 == 2) nb_up1_handoff_epilogue<MB, NBW, true>(ha_, acc, nzr, s_dco, s_bias, s_nst, wm * 64, wn * NBW, e_co0, e_n, e_y0, e_x0, lh, l31);
            else nb_up1_handoff_epilogue<MB, NBW, false>(ha_, acc, nzr, s_dco, s_bias, s_nst, wm * 64, wn * NBW, e_co0, e_n, e_y0, e_x0, lh, l31);
        } else nb_up1_handoff_epilogue<MB, NBW, false>(ha_, acc, nzr, s_dco, s_bias, s_nst, wm * 64, wn * NBW, e_co0, e_n, e_y0, e_x0, lh, l31);
        NB_TSTAMP(3);
        NB_TSTAMP(4);
        return;
    }
    if constexpr (MW == 1) {
        if (p.tg.c && !p.y && p.c_out % 8 == 0) {
            // ToRGB straight from the accumulators (nobody taps the fp32 activations): the lane holds 32 of its pixel's 64
            // channels (4 lh .. + 3 of every group), lane l + 32 the other 32; partial sums in the order of nb_torgb_dot
            // (j = the four registers of a group, summed over (mb, g)), then the two lane halves meet through one
            // v_permlane32_swap per output.  No LDS image, no barrier.
            const float clampv = p.clamp >= 0.f ? p.clamp : __builtin_inff();
            // (the gain through a vector register of its own: straight from the kernarg pair (alpha, gain) the packed `* gain` below broadcast
            //  the pair's HIGH dword through op_sel:[1,0] in the loop-less instantiations -- the form tests/test_abi.py bans)
            float gain_t = p.gain;
            asm volatile("" : "+v"(gain_t));
#pragma unroll
            for (int nb = 0; nb < NBW; ++nb) {
                const float nzg = nzr[nb] * gain_t;
                f32x4 s0, s1, s2;
                s0 = 0.f; s1 = 0.f; s2 = 0.f;
#pragma unroll
                for (int mb = 0; mb < MB; ++mb)
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const int col = mb * 32 + 8 * g + 4 * lh;
                        if (col < p.c_out) {
                            const f32x4 d4 = *reinterpret_cast<const f32x4*>(s_dco + col) * gain_t;
                            const f32x4 b4 = *reinterpret_cast<const f32x4*>(s_bias + col) * gain_t + nzg;
                            const f32x4 a4 = {acc[mb][nb][4 * g], acc[mb][nb][4 * g + 1], acc[mb][nb][4 * g + 2], acc[mb][nb][4 * g + 3]};
                            f32x4 t = __builtin_elementwise_fma(a4, d4, b4);
                            const f32x4 ta = t * p.alpha;
#pragma unroll
                            for (int i = 0; i < 4; ++i) t[i] = __builtin_amdgcn_fmed3f(__builtin_amdgcn_fmed3f(t[i], ta[i], __builtin_inff()), -clampv, clampv);
                            s0 = __builtin_elementwise_fma(t, *reinterpret_cast<const f32x4*>(s_tw + col), s0);
                            s1 = __builtin_elementwise_fma(t, *reinterpret_cast<const f32x4*>(s_tw + p.c_out + col), s1);
                            s2 = __builtin_elementwise_fma(t, *reinterpret_cast<const f32x4*>(s_tw + 2 * p.c_out + col), s2);
                        }
                    }
                float pk[3] = {(s0[0] + s0[1]) + (s0[2] + s0[3]), (s1[0] + s1[1]) + (s1[2] + s1[3]), (s2[0] + s2[1]) + (s2[2] + s2[3])};
                float a[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    // swap(x, 0): the lower lanes get (their own, the upper lanes') partial sums
                    unsigned u0 = __builtin_bit_cast(unsigned, pk[k]), u1 = 0;
                    nb_swap32(u0, u1);
                    a[k] = __builtin_bit_cast(float, u0) + __builtin_bit_cast(float, u1);
                }
                if (lh == 0) nb_torgb_pixel(p.tg, e_n, (e_y0 + wn * NBW + nb) * W + e_x0 + l31, a[0], a[1], a[2], s_tcol, s_tcol01);
            }
            NB_TSTAMP(3);
            NB_TSTAMP(4);
            return;
        }
    }
    float* ot = reinterpret_cast<float*>(smem_h3);               // [CO_WG][PIX_WG] floats (<= 128 KiB)
    // (the gain through a vector register of its own: read from the kernarg pair (alpha, gain) the SLP vectoriser pairs the two `* gain` below
    //  into a v_pk_mul_f32 with the gain broadcast through op_sel:[1,0] -- a swizzled packed form, see NB_NO_PACKED_F32 in nb_common.h)
    float gain_v = p.gain;
    asm volatile("" : "+v"(gain_v));
#pragma unroll
    for (int nb = 0; nb < NBW; ++nb) {
        const int trow = wn * NBW + nb;
        const float nzg = nzr[nb] * gain_v, clampv = p.clamp >= 0.f ? p.clamp : __builtin_inff();
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int col = wm * 64 + mb * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;      // c_out within the workgroup
                // (channels past c_out carry dco = bias = 0 and are never stored)
                ot[col * PIX_WG + trow * 32 + l31] = nb_h3_act(acc[mb][nb][r], s_dco[col] * gain_v, s_bias[col] * gain_v + nzg, p.alpha, clampv);
            }
        }
    }
    __syncthreads();
    NB_TSTAMP(3);
    if (p.tg.c) {
        // ToRGB on the tile while it sits in LDS: 3 dot products over the channels per pixel, then the triad tail
        for (int pix = tid; pix < PIX_WG; pix += 512) {
            float a0, a1, a2;
            nb_torgb_dot(p.c_out, s_tw, [&](int ch) { return ot[ch * PIX_WG + pix]; }, a0, a1, a2);
            nb_torgb_pixel(p.tg, e_n, (e_y0 + (pix >> 5)) * W + e_x0 + (pix & 31), a0, a1, a2, s_tcol, s_tcol01);
        }
        if (!p.y) return;
    }
    if (!(p.dbg & 1)) {
        constexpr int V4_PER_ROW = PIX_WG / 4;                   // float4 per c_out row
        for (int e = tid; e < CO_WG * V4_PER_ROW; e += 512) {
            const int col = e / V4_PER_ROW, q4 = e - col * V4_PER_ROW;
            const int co = e_co0 + col;
            if (co < p.c_out) {
                const int trow = q4 >> 3, px = (q4 & 7) * 4;
                const f32x4 v = *reinterpret_cast<const f32x4*>(ot + col * PIX_WG + q4 * 4);
                *reinterpret_cast<f32x4*>(p.y + ((size_t)e_n * p.c_out + co) * ((size_t)H * W) + (size_t)(e_y0 + trow) * W + e_x0 + px) = v;
            }
        }
    }
    NB_TSTAMP(4);
    };
    epilogue();
    if (item_next >= total) break;
    item = item_next;
    // every wave is through with the tile's tables (and, on the fp32-output path, with the staged tile)
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    NB_TSTAMP(0);
    if (!early) prologue_issue();
  }
#undef NB_TSTAMP
#define NB_TSTAMP(k)                                                                                         \
    do {                                                                                                     \
        if (p.tstamps && threadIdx.x == 0) p.tstamps[(size_t)(blockIdx.x + blockIdx.y * gridDim.x) * 8 + (k)] = __builtin_amdgcn_s_memrealtime(); \
    } while (0)
}

// ------------------------------------------------------------------------------------------------
// Small-workgroup form of the same layer: 4 waves, 64 c_out x 256 px, <= 75 KB of LDS, so TWO workgroups share a
// CU and one's prologue / epilogue (DMA latency, VALU, stores) runs under the other's MFMAs.  K loop = (16-channel
// chunk, tap row) steps, double buffered: the rows a step needs are gathered by LDS-DMA (zero page outside the
// image), the next step's DMA is in flight under the current step's MFMAs (the scheme of nb_encoder.hip).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256, 2) void modconv3x3_up1_h3s_kernel(const H3Params p) {
    if (p.out_f8) nb_set_fp16_ovfl();             // f8 hand-off: the fp8 (and f16) conversions saturate
    constexpr int NW = 4, MB = 2, NBW = 2, CO_WG = 64, TH = NW * NBW, PW = 34, PIX_WG = TH * 32;
    constexpr int SLOTS = TH * PW, PP = (SLOTS + 63) / 64, XPL = PP * 64, NXP = 4 * PP, NXPW = (NXP + NW - 1) / NW;
    constexpr int WSLOTS = 12 * CO_WG, NWP = WSLOTS / 64, NWPW = NWP / NW;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_h3[];
    h8* xbuf = reinterpret_cast<h8*>(smem_h3);                    // [2][4][XPL]
    h8* wbuf = xbuf + 2 * 4 * XPL;                                // [2][WSLOTS]
    const int tid = threadIdx.x;
    const int lane = tid & 63, wn = __builtin_amdgcn_readfirstlane(tid >> 6), lh = lane >> 5, l31 = lane & 31;
    const int H = p.h, W = p.w;
    int b = blockIdx.x;
    if (gridDim.x % 8 == 0 && p.slices > 1) b = (b & 7) * (gridDim.x >> 3) + (b >> 3);       // slices of a tile share an XCD
    const int slice = b % p.slices; b /= p.slices;
    const int tile_x = b % p.tiles_x; const int tile_y = b / p.tiles_x;
    const int n = blockIdx.y;
    const int y0 = tile_y * TH, x0 = tile_x * 32, co0 = slice * CO_WG;
    const size_t HW8 = (size_t)H * W * 8;
    const _Float16* xn = p.x + (size_t)n * p.c8 * 2 * HW8;

    __shared__ __attribute__((aligned(16))) float s_dco[CO_WG], s_bias[CO_WG], s_nst[CO_WG];
    __shared__ float s_tw[3 * 128], s_tcol[9], s_tcol01[9];
    if (tid < CO_WG) {
        const int co = co0 + tid;
        s_dco[tid] = co < p.c_out ? p.dcoefs[(size_t)n * p.c_out + co] : 0.f;
        s_bias[tid] = co < p.c_out ? p.bias[co] : 0.f;
        s_nst[tid] = (p.yh2 && co < p.c_out) ? p.next_styles[(size_t)n * p.next_stride + co] : 0.f;
    }
    if (p.tg.c) nb_torgb_setup(p.tg, n, s_tw, s_tcol, s_tcol01, tid, 256, blockIdx.x == 0);
    float nzr[NBW];
#pragma unroll
    for (int nb = 0; nb < NBW; ++nb)
        nzr[nb] = p.noise ? p.noise[(size_t)n * p.noise_stride_n + (size_t)(y0 + wn * NBW + nb) * W + x0 + l31] : 0.f;
    if (p.nsrc.const_t) {
        // the lane's pixels (row y0 + wn NBW + nb, column x0 + l31): column parameters once, row parameters per row
        float np0, np1, wy0, wy1;
        int sy0;
        nb_noise_np(p.nsrc, n, np0, np1);
        nb_noise_axis(p.nsrc, x0 + l31, np1, sy0, wy0, wy1);
        const float strength = p.nsrc.strength[0];
#pragma unroll
        for (int nb = 0; nb < NBW; ++nb) {
            float wx0, wx1;
            int sx0;
            nb_noise_axis(p.nsrc, y0 + wn * NBW + nb, np0, sx0, wx0, wx1);
            nzr[nb] = nb_noise_value(p.nsrc, strength, sx0, wx0, wx1, sy0, wy0, wy1);
        }
    }

    int xcol[NXPW], xrow[NXPW], xpl[NXPW], xdst[NXPW];
#pragma unroll
    for (int i = 0; i < NXPW; ++i) {
        const int q = i * NW + wn;                    // NXP = NW * NXPW exactly
        const int pl4 = q / PP, part = q - pl4 * PP;
        const int e = part * 64 + lane;
        const int r = e / PW, c = e - r * PW;
        const int gx = x0 - 1 + c;
        xpl[i] = pl4;
        xdst[i] = pl4 * XPL + part * 64;
        xrow[i] = y0 - 1 + r;
        xcol[i] = (e < SLOTS && gx >= 0 && gx < W) ? gx * 8 : -1;
    }
    auto issue = [&](int t, int buf) {                // t = chunk * 3 + ky
        const int c = t / 3, ky = t - 3 * c;
        h8* xd = xbuf + buf * 4 * XPL;
#pragma unroll
        for (int i = 0; i < NXPW; ++i) {
            const int cg = 2 * c + (xpl[i] >> 1), gy = xrow[i] + ky;
            const _Float16* src = reinterpret_cast<const _Float16*>(p.zeros);
            if (xcol[i] >= 0 && gy >= 0 && gy < H && cg < p.c8)
                src = xn + (size_t)(4 * c + xpl[i]) * HW8 + (size_t)gy * W * 8 + xcol[i];
            __builtin_amdgcn_global_load_lds(NB_GLOBAL_PTR(src), NB_LDS_PTR(xd + xdst[i]), 16, 0, 0);
        }
        h8* wd = wbuf + buf * WSLOTS;
#pragma unroll
        for (int i = 0; i < NWPW; ++i) {
            const int e = (i * NW + wn) * 64 + lane;
            const int row = e / CO_WG, j = e - row * CO_WG;                      // row = kx*4 + cg*2 + hl
            const _Float16* src = p.wts + (((size_t)t * 12 + row) * p.co_ld + co0 + j) * 8;
            __builtin_amdgcn_global_load_lds(NB_GLOBAL_PTR(src), NB_LDS_PTR(wd + (i * NW + wn) * 64), 16, 0, 0);
        }
    };

    f32x16 acc[MB][NBW];
#pragma unroll
    for (int mb = 0; mb < MB; ++mb)
#pragma unroll
        for (int nb = 0; nb < NBW; ++nb)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mb][nb][r] = 0.f;
    const int T = p.nchunks * 3;
    const int a_base = lh * 2 * CO_WG + l31;
    const int b_base = lh * 2 * XPL + (wn * NBW) * PW + l31;
    issue(0, 0);
    for (int t = 0; t < T; ++t) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        issue(t + 1 < T ? t + 1 : T - 1, (t + 1) & 1);
        __builtin_amdgcn_sched_barrier(0);
        const h8* xb = xbuf + (t & 1) * 4 * XPL;
        const h8* wb = wbuf + (t & 1) * WSLOTS;
        h8 ah[2][MB], al[2][MB], bh[2][NBW], bl[2][NBW];
        auto fetch = [&](int kx, h8 (&fah)[MB], h8 (&fal)[MB], h8 (&fbh)[NBW], h8 (&fbl)[NBW]) {
#pragma unroll
            for (int mb = 0; mb < MB; ++mb) {
                fah[mb] = wb[a_base + kx * 4 * CO_WG + mb * 32];
                fal[mb] = wb[a_base + kx * 4 * CO_WG + CO_WG + mb * 32];
            }
#pragma unroll
            for (int nb = 0; nb < NBW; ++nb) {
                fbh[nb] = xb[b_base + nb * PW + kx];
                fbl[nb] = xb[b_base + XPL + nb * PW + kx];
            }
        };
        fetch(0, ah[0], al[0], bh[0], bl[0]);
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int cu = kx & 1;
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[cu][0], bh[cu][0], acc[0][0], 0, 0, 0);
            if (kx + 1 < 3) fetch(kx + 1, ah[cu ^ 1], al[cu ^ 1], bh[cu ^ 1], bl[cu ^ 1]);
#pragma unroll
            for (int mb = 0; mb < MB; ++mb)
#pragma unroll
                for (int nb = 0; nb < NBW; ++nb) {
                    if (mb + nb > 0)
                        acc[mb][nb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[cu][mb], bh[cu][nb], acc[mb][nb], 0, 0, 0);
                    acc[mb][nb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[cu][mb], bl[cu][nb], acc[mb][nb], 0, 0, 0);
                    acc[mb][nb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[cu][mb], bh[cu][nb], acc[mb][nb], 0, 0, 0);
                }
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            if (kx + 1 < 3) __builtin_amdgcn_sched_group_barrier(0x100, 2 * MB + 2 * NBW, 0);
            __builtin_amdgcn_sched_group_barrier(0x008, 3 * MB * NBW - 1, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();                                  // staging buffers are dead from here on
    if (p.dbg & 4) { if (acc[0][0][0] == 123.456f) p.y[0] = 0.f; return; }      // ablation: main loop only

    if (p.yh2) {
        nb_up1_handoff_epilogue<MB, NBW>(nb_handoff_args(p.yh2, p.c8_next, p.c_out, p.h, p.w, p.out_f8, p.dbg, p.alpha, p.gain, p.clamp), acc, nzr, s_dco, s_bias, s_nst, 0, wn * NBW, co0, n, y0, x0, lh, l31);
        return;
    }
    float* ot = reinterpret_cast<float*>(smem_h3);               // [CO_WG][PIX_WG]
#pragma unroll
    for (int nb = 0; nb < NBW; ++nb) {
        const int trow = wn * NBW + nb;
        const float nzg = nzr[nb] * p.gain, clampv = p.clamp >= 0.f ? p.clamp : __builtin_inff();
#pragma unroll
        for (int mb = 0; mb < MB; ++mb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int col = mb * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                ot[col * PIX_WG + trow * 32 + l31] = nb_h3_act(acc[mb][nb][r], s_dco[col] * p.gain, s_bias[col] * p.gain + nzg, p.alpha, clampv);
            }
    }
    __syncthreads();
    if (p.tg.c) {
        for (int pix = tid; pix < PIX_WG; pix += 256) {
            float a0, a1, a2;
            nb_torgb_dot(p.c_out, s_tw, [&](int ch) { return ot[ch * PIX_WG + pix]; }, a0, a1, a2);
            nb_torgb_pixel(p.tg, n, (y0 + (pix >> 5)) * W + x0 + (pix & 31), a0, a1, a2, s_tcol, s_tcol01);
        }
        if (!p.y) return;
    }
    constexpr int V4_PER_ROW = PIX_WG / 4;
    for (int e = tid; e < CO_WG * V4_PER_ROW; e += 256) {
        const int col = e / V4_PER_ROW, q4 = e - col * V4_PER_ROW;
        const int co = co0 + col;
        if (co < p.c_out) {
            const int trow = q4 >> 3, px = (q4 & 7) * 4;
            const f32x4 v = *reinterpret_cast<const f32x4*>(ot + col * PIX_WG + q4 * 4);
            *reinterpret_cast<f32x4*>(p.y + ((size_t)n * p.c_out + co) * ((size_t)H * W) + (size_t)(y0 + trow) * W + x0 + px) = v;
        }
    }
}

#define NB_PERSIST_WGS_PER_CU 4
// Workgroups per CU of the persistent launches (both large kernels).  1 would keep every workgroup resident from the start; with 4 a
// workgroup still walks 2-4 tiles of the BASELINE launches (the prefetch pays from the second tile on) but CUs come free four times per
// launch, which is what lets another stream's kernels in: same-box, 3 streams in flight, 18 415 (1) / 18 490 (2) / 18 577 (4) patches/s
// against 18 311 with one workgroup per tile; on ONE stream all three give +2.8 % (profiles/r06_ab_persistent_grid.txt).
int g_persist_wgs_per_cu = NB_PERSIST_WGS_PER_CU;
// developer / test hook: <= 0 restores the default
extern "C" void nb_debug_set_persistent_wgs_per_cu(int k) { g_persist_wgs_per_cu = k > 0 ? k : NB_PERSIST_WGS_PER_CU; }
static int g_up1_persist = -1;
// developer / test hook: 1 = persistent workgroups of the 8-wave up=1 kernel (next tile's prologue ahead of the epilogue), -1 (default) / 0 = one workgroup per tile
extern "C" void nb_debug_set_up1_persistent(int mode) { g_up1_persist = mode; }

static int launch_h3s(H3Params p, int n, hipStream_t st) {
    constexpr size_t lds_stage = (size_t)2 * (4 * 320 + 12 * 64) * 16, lds_h2 = (size_t)2 * 256 * 72 * 2;
    const size_t lds = p.yh2 ? lds_h2 : lds_stage;
    p.tiles_x = p.w / 32; p.tiles_y = p.h / 8; p.slices = (p.c_out + 63) / 64;
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute((const void*)modconv3x3_up1_h3s_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_h2);
        attr_set = true;
    }
    hipLaunchKernelGGL(modconv3x3_up1_h3s_kernel, dim3(p.tiles_x * p.tiles_y * p.slices, n), dim3(256), lds, st, p);
    NB_CHECK_LAUNCH("modconv3x3_up1_h3s");
    return NB_OK;
}

template <int MW, bool F8 = false, int NBW = 2, bool V2 = false, bool F6 = false, bool PP = false, bool HO = false, bool PERSIST = true>
static int launch_h3(H3Params p, int n, hipStream_t st) {
    constexpr int NWN = 8 / MW, TH = NWN * NBW, CO_WG = MW * 64;
    constexpr int SLOTS = (TH + 2) * 34, XPL = ((SLOTS + 63) / 64) * 64;
    constexpr size_t lds_stage = (size_t)(2 * 4 * XPL + 4 * 12 * CO_WG) * 16, lds_h2 = (size_t)2 * TH * 32 * (CO_WG + 8) * 2;
    const size_t lds = lds_stage > lds_h2 ? lds_stage : lds_h2;
    p.tiles_x = p.w / 32; p.tiles_y = p.h / TH; p.slices = (p.c_out + CO_WG - 1) / CO_WG;
    p.items_x = p.tiles_x * p.tiles_y * p.slices; p.items = p.items_x * n;
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute((const void*)modconv3x3_up1_h3_kernel<MW, F8, NBW, V2, F6, PP, HO, PERSIST>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        attr_set = true;
    }
    // persistent workgroups: one per CU (fewer items than CUs: one each), the next tile's prologue issued ahead of the current tile's
    // epilogue; g_up1_persist == 0 (test hook): one workgroup per item, as until round 5
    const long want = (long)nb_num_cus() * g_persist_wgs_per_cu;                 // (workgroups per CU: see NB_PERSIST_WGS_PER_CU)
    dim3 grid(PERSIST && p.items > want ? (unsigned)want : (unsigned)p.items);
    hipLaunchKernelGGL((modconv3x3_up1_h3_kernel<MW, F8, NBW, V2, F6, PP, HO, PERSIST>), grid, dim3(512), lds, st, p);
    NB_CHECK_LAUNCH("modconv3x3_up1_h3");
    return NB_OK;
}

static int g_force_up1_v2 = -1;
// developer / test hook: -1 = automatic (on), 0 / 1 = the round-3 / the software-pipelined K loop of the f8 up=1 kernel
extern "C" void nb_debug_set_up1_v2(int mode) { g_force_up1_v2 = mode; }
#ifndef NB_UP1_PP_DEFAULT
#define NB_UP1_PP_DEFAULT 1          // round 5: +1.0 % / +0.5 % per step on a slow / fast box (three alternating pairs each), bit-identical
#endif
static int g_force_up1_pp = -1;
// developer / test hook: -1 = automatic, 0 / 1 = the software-pipelined / the ping-pong K loop of the f8 up=1 kernel
extern "C" void nb_debug_set_up1_pp(int mode) { g_force_up1_pp = mode; }
static int g_force_nbw = 0;
// developer / test hook: 0 = automatic, 1 / 2 = force that many 32-pixel rows per wave in the 8-wave up=1 kernel
extern "C" void nb_debug_set_up1_rows(int nbw) { g_force_nbw = nbw; }
static int g_force_up1_small = -1;
// developer / test hook: -1 = automatic (images <= 32 x 32), 0 / 1 = never / always the 4-wave two-workgroups-per-CU form of the H2 up=1 kernel
extern "C" void nb_debug_set_up1_small(int mode) { g_force_up1_small = mode; }

// workgroups of a full-height launch of the 8-wave kernel: 128 c_out x 8 rows of 32 pixels above 64 channels, else 64 x 16 rows
static long long nb_up1_h3_wgs(int n, int h, int w, int c_out) {
    const int mw = c_out > 64 ? 2 : 1;
    return (long long)n * (w / 32) * (h / (16 / mw)) * ((c_out + 64 * mw - 1) / (64 * mw));
}

static int nb_up1_h3_impl(const H3ConvArgs& a, void* stream, const TorgbParams* tg = nullptr, int in_fmt = 0) {
    const int n = a.n, h = a.h, w = a.w, c_out = a.c_out, out_fmt = a.out_fmt;
    const bool f8 = in_fmt != 0, f6 = in_fmt == 2;          // (the f6 form is a variant of the f8 loop: same containers, same staging)
    const bool hi_only = in_fmt == 3;                       // f8 containers, correction products skipped (conv_mode "f16": where the ping-pong loop runs)
    NB_REQUIRE(out_fmt == 0 || ((out_fmt == 1 || out_fmt == 2) && a.y_h2 && c_out % 16 == 0 && a.c_next % 16 == 0),
               "modconv3x3_up1_h3: f8 / f6 output needs an H2 destination and c_out, c_next %% 16 == 0");
    NB_REQUIRE(a.x_h2 && a.w_h3 && a.dcoefs && a.bias && (tg ? !a.y_h2 : ((a.y != nullptr) != (a.y_h2 != nullptr))), "modconv3x3_up1_h3: null pointer");
    NB_REQUIRE(!f8 || a.c_in % 16 == 0, "modconv3x3_up1_h3: the f8 operand format needs c_in %% 16 == 0 (got %d)", a.c_in);
    H3Params p;
    if (const int rc = nb_h3_launch_setup(p, "modconv3x3_up1_h3", a, 1, w % 32 == 0 && h % 16 == 0, "w % 32 == 0 and h % 16 == 0", true)) return rc;
    p.tg = TorgbParams{};
    if (tg) p.tg = *tg;
    const long long wgs_full = nb_up1_h3_wgs(n, h, w, c_out);
    p.tstamps = g_tstamps && wgs_full <= g_tstamps_cap ? g_tstamps : nullptr;
    // the 4-wave / 2-workgroups-per-CU form wins on small images (fewer, larger workgroups leave CUs idle there); on the
    // large layers both forms run at the same rate -- the chip is power-limited in these loops, not latency-limited
    { const bool small = g_force_up1_small >= 0 ? g_force_up1_small != 0 : (h * w <= 32 * 32);
      if (small && !f8 && (!tg || c_out <= 64)) return launch_h3s(p, n, (hipStream_t)stream); }
    // half-height tiles when the full ones leave the chip mostly idle (batch 1); g_force_nbw: test hook
    const bool half = g_force_nbw ? g_force_nbw == 1 : wgs_full < 160;
    hipStream_t st = (hipStream_t)stream;
    // the software-pipelined K loop (V2; both operand formats) unless switched off (test hook nb_debug_set_up1_v2)
    // (its pieces walk the chunks with a fixed per-chunk stride: whole 16-channel chunks only -- f8 operands always are; H2 operands
    //  with an odd number of channel groups keep the round-3 loop, whose last chunk reads the missing group from the zero page)
    const bool v2 = g_force_up1_v2 != 0 && (f8 || p.c8 % 2 == 0);
    NB_REQUIRE(out_fmt != 2 || (f8 && v2), "modconv3x3_up1_h3: the f6 output format is written by the software-pipelined f8 / f6 kernels only");
    // Persistent workgroups: automatic = NO (see the kernel's PERSIST); nb_debug_set_up1_persistent(1) = always -- the tests and
    // tools/stress_persistent.py keep that instantiation honest.  Half-height launches (< 160 workgroups) have nothing to walk: loop-less always.
    const bool persist = g_up1_persist > 0;
    // the ping-pong form of the f8 loop (full-height tiles): nb_debug_set_up1_pp
    const bool pp = (g_force_up1_pp >= 0 ? g_force_up1_pp : NB_UP1_PP_DEFAULT) != 0;
    using T = std::true_type; using F = std::false_type;
    using I1 = std::integral_constant<int, 1>; using I2 = std::integral_constant<int, 2>;
    auto go1 = [&](auto mw_, auto nbw_, auto f8_, auto v2_, auto f6_, auto pp_, auto ho_) {
        constexpr int MW_ = decltype(mw_)::value, NBW_ = decltype(nbw_)::value;
        constexpr bool F8_ = decltype(f8_)::value, V2_ = decltype(v2_)::value, F6_ = decltype(f6_)::value, PP_ = decltype(pp_)::value, HO_ = decltype(ho_)::value;
        if constexpr (NBW_ == 2) {
            if (persist) return launch_h3<MW_, F8_, NBW_, V2_, F6_, PP_, HO_, true>(p, n, st);
        }
        return launch_h3<MW_, F8_, NBW_, V2_, F6_, PP_, HO_, false>(p, n, st);
    };
    auto go = [&](auto nbw_, auto f8_, auto v2_, auto f6_, auto pp_, auto ho_) {
        return c_out > 64 ? go1(I2{}, nbw_, f8_, v2_, f6_, pp_, ho_) : go1(I1{}, nbw_, f8_, v2_, f6_, pp_, ho_);
    };
    auto go_rows = [&](auto f8_, auto v2_, auto f6_) { return half ? go(I1{}, f8_, v2_, f6_, F{}, F{}) : go(I2{}, f8_, v2_, f6_, F{}, F{}); };
    if (f6) return go_rows(T{}, T{}, T{});                  // (the software-pipelined loop only)
    if (!half && f8 && v2 && pp) return hi_only ? go(I2{}, T{}, T{}, F{}, T{}, T{}) : go(I2{}, T{}, T{}, F{}, T{}, F{});
    if (f8) return v2 ? go_rows(T{}, T{}, F{}) : go_rows(T{}, F{}, F{});
    return v2 ? go_rows(F{}, T{}, F{}) : go_rows(F{}, F{}, F{});
}

// NbTorgbArgs of an entry point -> the fused epilogue's TorgbParams (x stays null: it reads the accumulators).  `name` = the entry's
// message prefix.  (nb_torgb_triad_f32 of nb_ops.hip takes its arguments one by one, not as NbTorgbArgs: it fills its own.)
static int nb_up1_torgb_params(const char* name, const NbTorgbArgs* t, int c_out, int h, int w, TorgbParams* tg) {
    NB_REQUIRE(c_out <= 128, "%s: the fused ToRGB needs all channels in one workgroup (c_out <= 128)", name);
    NB_REQUIRE(t->styles_stride_n >= c_out + 9, "torgb_triad: styles rows must hold 9 color scalars + c styles");
    NB_REQUIRE(t->render_mode == 0 || t->render_mode == 1, "Unknown render mode for TriadGanPaintEngine: %d", t->render_mode);
    tg->x = nullptr; tg->styles = t->styles; tg->w = t->w; tg->bias = t->bias; tg->color_bias = t->color_bias;
    tg->logits = t->logits; tg->uvs = t->uvs; tg->img = t->img; tg->colors_out = t->colors_out; tg->user_colors = t->user_colors;
    tg->sfactor = t->sfactor; tg->rgba_f32 = t->rgba_f32; tg->rgba_u8 = t->rgba_u8;
    tg->styles_stride_n = t->styles_stride_n; tg->c = c_out; tg->hw = h * w; tg->render_mode = t->render_mode; tg->clamp = t->clamp;
    return NB_OK;
}

extern "C" int nb_modconv3x3_up1_h3_ex(const void* x, int c_in, const void* wts, const float* dcoefs, const float* noise,
                                      int64_t noise_stride_n, const float* bias, float* y_f32, void* y_h2,
                                      const float* next_styles, int next_stride, int c_next, const NbTorgbArgs* t, int in_fmt,
                                      int out_fmt, int n, int h, int w, int c_out, float alpha, float gain, float clamp,
                                      void* stream) {
    NB_REQUIRE(in_fmt >= 0 && in_fmt <= 3, "modconv3x3_up1_h3: operand format must be 0 (H2), 1 (f8), 2 (f6) or 3 (f8 containers, hi x hi products only)");
    if (!t)
        return nb_up1_h3_impl({x, c_in, wts, dcoefs, noise, noise_stride_n, bias, y_f32, y_h2, next_styles, next_stride, c_next, n, h, w, c_out, alpha, gain, clamp, out_fmt},
                              stream, nullptr, in_fmt);
    NB_REQUIRE(t->styles && t->w && t->bias && t->color_bias && !y_h2, "modconv3x3_up1_h3_ex: bad ToRGB arguments");
    TorgbParams tg;
    if (const int rc = nb_up1_torgb_params("modconv3x3_up1_h3_ex", t, c_out, h, w, &tg)) return rc;
    return nb_up1_h3_impl({x, c_in, wts, dcoefs, noise, noise_stride_n, bias, y_f32, nullptr, nullptr, 0, 0, n, h, w, c_out, alpha, gain, clamp, 0}, stream, &tg, in_fmt);
}

extern "C" int nb_modconv3x3_up1_h3(const void* x_h2, int c_in, const void* w_h3, const float* dcoefs, const float* noise,
                                    int64_t noise_stride_n, const float* bias, float* y, int n, int h, int w, int c_out,
                                    float alpha, float gain, float clamp, void* stream) {
    return nb_up1_h3_impl({x_h2, c_in, w_h3, dcoefs, noise, noise_stride_n, bias, y, nullptr, nullptr, 0, 0, n, h, w, c_out, alpha, gain, clamp, 0}, stream);
}

extern "C" int nb_modconv3x3_up1_h3_torgb(const void* x_h2, int c_in, const void* w_h3, const float* dcoefs, const float* noise,
                                          int64_t noise_stride_n, const float* bias, float* y, int n, int h, int w, int c_out,
                                          float alpha, float gain, float clamp, const NbTorgbArgs* t, void* stream) {
    NB_REQUIRE(t && t->styles && t->w && t->bias && t->color_bias, "modconv3x3_up1_h3_torgb: null pointer");
    TorgbParams tg;
    if (const int rc = nb_up1_torgb_params("modconv3x3_up1_h3_torgb", t, c_out, h, w, &tg)) return rc;
    return nb_up1_h3_impl({x_h2, c_in, w_h3, dcoefs, noise, noise_stride_n, bias, y, nullptr, nullptr, 0, 0, n, h, w, c_out, alpha, gain, clamp, 0}, stream, &tg);
}

extern "C" int nb_modconv3x3_up1_h3_h2(const void* x_h2, int c_in, const void* w_h3, const float* dcoefs, const float* noise,
                                       int64_t noise_stride_n, const float* bias, const float* next_styles, int next_stride,
                                       void* y_h2, int c_next, int n, int h, int w, int c_out, float alpha, float gain,
                                       float clamp, void* stream) {
    return nb_up1_h3_impl({x_h2, c_in, w_h3, dcoefs, noise, noise_stride_n, bias, nullptr, y_h2, next_styles, next_stride, c_next, n, h, w, c_out, alpha, gain, clamp, 0}, stream);
}
