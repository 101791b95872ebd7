// ------------------------------------------------------------------------------------------------
// up = 2 on the f16 matrix cores: the 4-phase transposed convolution + fused polyphase FIR of
// nb_modconv.hip (same math, same quad grid: see the comment block there), with split-f16 products.
//
// Workgroup = 8 waves, one 12 x 32 quad tile (14 x 34 = 476 halo'd positions = 15 MFMA column blocks of 32, two
// per wave) x 32 c_out.  All four phases share the staged halo tile (9 taps per staged byte), so every wave
// carries 2 blocks x 4 phases x 16 = 128 accumulator registers; the A/B fragments are streamed per tap.
// (12 rows do not divide the image height: the last tile row overhangs and is masked.)  Input H2 (pre-modulated), weights [chunk][tap 9][cg 2][hi/lo 2][c_out_ld][8], output fp32 NCHW.
// ------------------------------------------------------------------------------------------------
#include "nb_h3_launch.h"

#ifndef NB_H3_TQH
#define NB_H3_TQH 12
#endif
#define NB_H3_TQH_SMALL 5       // tile height of the under-filled (batch-1) launches
#define NB_H3_TQH_MID 8         // 10 x 34 = 340 positions = 11 blocks (3 / 3 / 3 / 2 per SIMD): for launches whose 12-row tiles end in a mostly empty round of workgroups
#define NB_H3_STAGES 3          // LDS-DMA stages of the up=2 kernel (planes at their exact size: 3 x 52 032 B for the 12-row tile)

// TQH = quad rows per tile: NB_H3_TQH (12) for throughput; 5 (7 x 34 = 238 positions = 8 column blocks, one per wave)
// when the large tiles would leave most of the chip idle - the batch-1 / interactive configuration.
// OUTM = output mode: 0 = fp32 NCHW, 1 = the consumer's H2 tensor, 2 = the consumer's tensor in the "f8" operand format.
// TQW_ = quad columns per tile: 32, or 16 for 16-wide inputs (b32.conv0 at large batch: 8 x 16 tiles = 10 x 18 = 180
// positions = 6 blocks, one per wave).
// (Tried and dropped, DESIGN.md 6: a one-wave-per-SIMD form with 256 accumulators per wave and a hand-ordered K loop, and two
//  4-wave workgroups per CU on 5-row tiles -- neither was faster.)
// NW_ / NST_ = waves per workgroup / LDS-DMA stages: 8 / 3 (one workgroup per CU), or 4 / 2 on 12 x 16 tiles (14 x 18 = 252
// positions = 8 column blocks, two per wave; 2 x 36.7 KB of staging) so that TWO workgroups share a CU and one's prologue
// (first-chunk DMA latency) and epilogue (LDS round trip, FIR, conversions, stores: a quarter to a third of a workgroup's
// life, no matrix work) run under the other's K loop.
template <bool F8, int TQH, int OUTM = 0, int TQW_ = 32, int NW_ = 8, int NST_ = NB_H3_STAGES>
__global__ __launch_bounds__(NW_ * 64, 2) void modconv3x3_up2_h3_kernel(const H3Up2Params p) {
    NB_TSTAMP(0);
    if constexpr (OUTM == 2) nb_set_fp16_ovfl();
    nb_stagger(p.stagger_ticks, 256);
    constexpr int NW = NW_, NT = NW_ * 64, TQW = TQW_, PH = TQH + 2, PW = TQW + 2, NPOS = PH * PW;     // 476
    constexpr int NBLK = (NPOS + 31) / 32;            // 15 position blocks
    constexpr int NBJ = (NBLK + NW - 1) / NW;         // blocks per wave (2)
    constexpr int XR = TQH + 3, XS = TQW + 3;         // halo tile 15 x 35 input pixels
    // planes are packed at their exact size (the last 1-KiB DMA piece of a plane is partial: lanes past the plane do not
    // copy), which is what lets THREE stages of the 12-row tile fit the 160 KiB of LDS
    constexpr int SLOTS = XR * XS, PP = (SLOTS + 63) / 64, XPL = SLOTS;         // 525 slots -> 9 pieces
    constexpr int NXP = 4 * PP, NXPW = (NXP + NW - 1) / NW;                     // 36 -> 5 per wave
    constexpr int WSLOTS = 36 * 32, NWP = WSLOTS / 64, NWPW = (NWP + NW - 1) / NW;   // 18 -> 3 per wave
    // LDS-DMA pieces a wave issues per chunk: the 36 activation + 18 weight pieces are ONE list dealt round-robin to the waves
    // (7 each, 2 re-copies; dealt per kind it was 5 + 3 = 8 each with 10 re-copies -- and a piece is a KiB through the CU's
    // vector-memory path whether anybody needs it or not)
    constexpr int NPC = (NXP + NWP + NW - 1) / NW;
    constexpr int STAGE = 4 * XPL + WSLOTS;           // 16-byte slots per stage
    constexpr int NST = NST_;                         // 3 (2: the two-workgroups-per-CU form)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_h3[];
    h8* ring = reinterpret_cast<h8*>(smem_h3);        // [NST][ x: 4 planes x XPL | w: 36 rows x 32 ]

    const int tid = threadIdx.x;
    const int lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6), lh = lane >> 5, l31 = lane & 31;
    const int H = p.h, W = p.w;
    int b = blockIdx.x;
    // XCD-aware order: consecutive workgroup ids go round-robin to the 8 XCDs (each with its own L2), so the c_out
    // slices of one input tile -- which re-read the same activations -- are renumbered to share an XCD
    // (the XCD's share of the tile list rotates with the sample: the cheap tiles of a ragged last tile row -- see the K loop's
    //  copies below -- would otherwise all sit on the last XCDs, which then idle while the others finish)
    if (gridDim.x % 8 == 0 && !(p.dbg & 8)) b = (((b & 7) + blockIdx.y) & 7) * (gridDim.x >> 3) + (b >> 3);
    const int slice = b % p.slices; b /= p.slices;
    const int tile_x = b % p.tiles_x; const int tile_y = b / p.tiles_x;
    const int n = blockIdx.y;
    const int I0 = tile_y * TQH, J0 = tile_x * TQW;
    const int co0 = slice * 32;
    const size_t HW8 = (size_t)H * W * 8;
    const _Float16* xn = p.x + (size_t)n * p.c8 * 2 * HW8;
    const int nblk = wv < NBLK - (NBJ - 1) * NW ? NBJ : NBJ - 1;      // blocks wv, wv+8 (< 15)

    // epilogue operands fetched under the prologue DMA: demodulation / bias per channel and the tile's noise
    __shared__ __attribute__((aligned(16))) float s_dco[32], s_bias[32], s_nst[32];
    __shared__ __attribute__((aligned(16))) float s_noise[2 * TQH * 2 * TQW];
    if (tid < 32) {
        const int co = co0 + tid;
        // the activation gain is folded into the three addends: lrelu(g t) = g lrelu(t) for g > 0 (the launcher checks)
        float dg = co < p.c_out ? p.dcoefs[(size_t)n * p.c_out + co] * p.gain : 0.f;
        float bv = co < p.c_out ? p.bias[co] : 0.f;
        // (the two `* gain` must not meet in one packed instruction: the SLP vectoriser pairs them as v_pk_mul_f32 with the gain
        //  broadcast through op_sel:[1,0] in some instantiations -- a swizzled packed form, see NB_NO_PACKED_F32 in nb_common.h)
        asm volatile("" : "+v"(dg), "+v"(bv));
        s_dco[tid] = dg;
        s_bias[tid] = bv * p.gain;
        s_nst[tid] = (p.yh2 && co < p.c_out) ? p.next_styles[(size_t)n * p.next_stride + co] : 0.f;
    }
    // LDS-DMA descriptors of this wave's pieces.  Activation piece i: plane xpl (= cg_local*2 + hi/lo), 64 slots from
    // `part`; xsp = element offset of the lane's source slot inside a plane (-1: outside the image -> zero page),
    // xok = the lane's slot belongs to the plane (the last piece of a plane is partial)
    int xsp[NXPW], xpl[NXPW], xdst[NXPW];
    bool xok[NXPW];
#pragma unroll
    for (int i = 0; i < NXPW; ++i) {
        int q = i * NW + wv;
        q = q < NXP ? q : NXP - 1;
        const int pl = q / PP, part = q - pl * PP;
        const int e = part * 64 + lane;
        xpl[i] = pl;
        xdst[i] = pl * XPL + part * 64;
        xsp[i] = -1;
        xok[i] = e < SLOTS;
        if (e < SLOTS) {
            const int r = e / XS, c = e - r * XS;
            const int gy = I0 - 1 + r, gx = J0 - 1 + c;
            if (gy >= 0 && gy < H && gx >= 0 && gx < W) xsp[i] = (gy * W + gx) * 8;
        }
    }
    // piece k of chunk c into stage st: k < NXPW activations, else weights
    auto issue_piece = [&](auto kk, int c, h8* st) {
        constexpr int k = decltype(kk)::value;
        // list position u = k NW + wv: activation piece u (descriptor k of this wave) if u < NXP, else weight piece u - NXP
        constexpr bool ALLX = k * NW + NW - 1 < NXP, ALLW = k * NW >= NXP;
        const _Float16* xsrc = reinterpret_cast<const _Float16*>(p.zeros);
        h8* xd = st;
        bool xo = false;
        if constexpr (!ALLW) {
            const int cg = 2 * c + (xpl[k] >> 1);
            if (xsp[k] >= 0 && cg < p.c8) xsrc = xn + (size_t)(4 * c + xpl[k]) * HW8 + xsp[k];
            xd = st + xdst[k]; xo = xok[k];
        }
        if constexpr (ALLX) {
            if (xo) nb_lds_dma16(xsrc, xd);
        } else {
            int q = k * NW + wv - NXP;
            q = q < 0 ? 0 : (q < NWP ? q : NWP - 1);
            const int e = q * 64 + lane;
            const int row = e >> 5, j = e & 31;           // row = tap*4 + cg*2 + hl
            const _Float16* wsrc = p.wts + (((size_t)c * 36 + row) * p.co_ld + co0 + j) * 8;
            h8* wd = st + 4 * XPL + q * 64;
            if constexpr (ALLW) {
                nb_lds_dma16(wsrc, wd);
            } else {                                      // the round where the list changes kind: a wave issues ONE of the two (the
                const bool isx = k * NW + wv < NXP;       // other has no lane enabled, and such an instruction does not exist for vmcnt)
                if (isx && xo) nb_lds_dma16(xsrc, xd);
                if (!isx) nb_lds_dma16(wsrc, wd);
            }
        }
    };
    auto issue = [&](int c, h8* st) { nb_static_for<0, NPC>([&](auto k) { issue_piece(k, c, st); }); };
    // the pieces of one chunk spread over S points of the MFMA stream: point s issues pieces [s NPC / S, (s+1) NPC / S)
    auto issue_at = [&](auto ss, auto SS, int c, h8* st) {
        constexpr int s_ = decltype(ss)::value, S_ = decltype(SS)::value;
        nb_static_for<s_ * NPC / S_, (s_ + 1) * NPC / S_>([&](auto k) { issue_piece(k, c, st); });
    };

    // B-fragment base slots: position (r, c) of block (wv + 8j); X(r, c) = slot r*XS + c of plane (lh*2 + hl)
    int boff[NBJ];
#pragma unroll
    for (int j = 0; j < NBJ; ++j) {
        int pidx = (wv + NW * j) * 32 + l31;
        pidx = pidx < NPOS ? pidx : NPOS - 1;
        const int r = pidx / PW, c = pidx - r * PW;
        boff[j] = lh * 2 * XPL + r * XS + c;
    }
    const int aoff = 4 * XPL + lh * 2 * 32 + l31;     // + tap*128 + hl*32

    f32x16 acc[NBJ][4];
#pragma unroll
    for (int j = 0; j < NBJ; ++j)
#pragma unroll
        for (int ph = 0; ph < 4; ++ph)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[j][ph][r] = 0.f;

    // ---- K loop: 16-channel chunks through a THREE-stage LDS ring.  Chunk c is read from stage c % 3 while the LDS-DMA
    //      pieces of chunk c+2 are issued one or two at a time BETWEEN the chunk's MFMA groups (a piece costs the issuing
    //      wave ~60 cycles among MFMAs, 100-185 in a burst next to the fragment reads -- and after a barrier both waves of a
    //      SIMD would burst at the same moment, with nobody feeding the matrix pipe: that burst was a third of the K loop
    //      of the 2-stage form).  One wait + barrier per chunk: vmcnt(NPC) = everything but the pieces just issued, i.e.
    //      chunk c+1 (issued a whole chunk ago) has landed; the barrier also frees stage (c-1) % 3 = (c+2) % 3 for the
    //      next chunk's pieces.  The last two chunks issue nothing (own copies of the body: no branch inside it). ----
    const int NC = p.nchunks;
    static_assert(NST == 3 || NST == 2, "ring indices below are written for three (or two) stages");
    issue(0, ring);
    // the tile's noise values (epilogue operand), computed or fetched while chunk 0 is on its way: with the in-kernel noise
    // (NbNoiseSrc) that is ~150 VALU instructions per thread, which cost 1 us of prologue when they ran ahead of the first DMA
    for (int e = tid; e < 2 * TQH * 2 * TQW; e += NT) {
        const int r = e / (2 * TQW), c = e - r * (2 * TQW);
        const int oy = 2 * I0 + r, ox = 2 * J0 + c;
        float v = (p.noise && oy < 2 * H) ? p.noise[(size_t)n * p.noise_stride_n + (size_t)oy * (2 * W) + ox] : 0.f;
        if (p.nsrc.const_t && oy < 2 * H) {
            float np0, np1, wx0, wx1, wy0, wy1;
            int sx0, sy0;
            nb_noise_np(p.nsrc, n, np0, np1);
            nb_noise_axis(p.nsrc, oy, np0, sx0, wx0, wx1);
            nb_noise_axis(p.nsrc, ox, np1, sy0, wy0, wy1);
            v = nb_noise_value(p.nsrc, p.nsrc.strength[0], sx0, wx0, wx1, sy0, wy0, wy1);
        }
        s_noise[e] = v * p.gain;
    }

    if (NC > 1 && NST == 3) {
        issue(1, ring + STAGE);
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NPC) : "memory");
    } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __builtin_amdgcn_s_barrier();
    NB_TSTAMP(1);
    // tap (a,b) row-major -> (slot offset of its input pixel, output phase): x11 = X(r,c), x10 = X(r,c+1),
    // x01 = X(r+1,c), x00 = X(r+1,c+1).  Only four distinct offsets occur, so the taps are walked grouped by offset:
    // one pair of B fragments (hi, lo) per block serves up to four taps, and the A fragments of the next tap (and the
    // B fragments of the next group) are fetched under the six MFMAs of the current tap.
    constexpr int kOrd[9] = {4, 5, 7, 8, 3, 6, 1, 2, 0};
    constexpr int kDel[9] = {0, 0, 0, 0, 1, 1, XS, XS, XS + 1};          // slot offset, in walk order
    constexpr int kGrp[9] = {0, 0, 0, 0, 1, 1, 2, 2, 3};
    constexpr int kPha[9] = {3, 2, 1, 0, 2, 0, 1, 0, 0};                 // kTapPhase[kOrd[i]]
    unsigned long long t_dma = 0, t_bar = 0;
    const unsigned long long t_loop0 = p.tstamps ? __builtin_amdgcn_s_memtime() : 0;
    // one chunk: reads from `st`; DMA = issue the pieces of chunk cn into `sn` between the MFMA groups
    // (Measured, round 3 -- an ablation build without the in-loop pieces, and one that also drops the barrier: the pieces cost
    //  ~480 of a chunk's ~3 550 cycles wherever they sit in the chunk, also with the two waves of a SIMD issuing theirs at
    //  different points; the barrier costs nothing; the loop without DMA still needs ~3 050 cycles for 2 432 cycles of MFMA.
    //  A variant with masked out-of-image lanes and pre-zeroed halo slots saved registers but is WRONG: a piece whose lanes
    //  are all masked is skipped, and the counted vmcnt waits below rely on every wave issuing exactly NPC pieces per chunk.)
    auto chunk = [&](auto dma_, auto nbe_, const h8* st, int cn, h8* sn) {
        constexpr bool DMA = decltype(dma_)::value;
        constexpr int NBE = decltype(nbe_)::value & 3;      // column blocks this wave multiplies (a wave whose second block does not exist skips its MFMAs and reads)
        // ... and how many of them take all four phases.  The LAST block of a full tile lies wholly in the last halo row
        // (positions 448 .. 475 of the 14 x 34), which the FIR reads in the odd-row phases only (oe, oo: rows ti .. ti+2 of a quad;
        // ee, eo: ti, ti+1): its six even-row taps and their fragment reads are left out (nbe_ & 4).
        constexpr int NB01 = (decltype(nbe_)::value & 4) ? NBE - 1 : NBE;
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (F8) {
            // "f8" operands (see modconv3x3_up1_h3_kernel): one f16 MFMA per tap for the main product, and the two
            // correction products of a PAIR of taps that feed the same output phase on one block-scaled fp8 MFMA:
            //   phase 0 (ee): taps (8,6) and (2,0)   phase 1 (eo): (7,1)   phase 2 (oe): (5,3)   phase 3 (oo): 4 alone
            // walked so that the B fragments of input offsets 0 and 1 are loaded once and those of XS / XS+1 replace them.
            const int sa = lh ? 116 : 127, sb = lh ? 129 : 118;
            const h8 z8 = {};
            h8 b0h[NBJ] = {}, b0l[NBJ] = {}, b1h[NBJ] = {}, b1l[NBJ] = {}, b2h[NBJ] = {}, b2l[NBJ] = {};
            h8 a1h = {}, a1l = {}, a2h = {}, a2l = {}, n1h = {}, n1l = {}, n2h = {}, n2l = {};
            using S4 = std::integral_constant<int, 4>;
#ifdef NB_ABL_NOREAD      // developer ablation (tools/build_variant.sh; timing only, wrong results): no fragment reads
#define NB_RD(dst, src) asm volatile("" : "+v"(dst))
#else
#define NB_RD(dst, src) dst = (src)
#endif
#define NB_LDA(tap, hi, lo) { NB_RD(hi, st[aoff + (tap) * 128]); NB_RD(lo, st[aoff + (tap) * 128 + 32]); }
#define NB_LDB(del, hi, lo) { _Pragma("unroll") for (int j = 0; j < NB01; ++j) { NB_RD(hi[j], st[boff[j] + (del)]); NB_RD(lo[j], st[boff[j] + XPL + (del)]); } }
#define NB_PAIR(ph, ah_a, al_a, bha, bla, ah_b, al_b, bhb, blb)                                                                   \
            { _Pragma("unroll") for (int j = 0; j < ((ph) >= 2 ? NBE : NB01); ++j) {                                               \
                f32x16& a_ = acc[j][ph];                                                                                           \
                a_ = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah_a, bha[j], a_, 0, 0, 0);                                            \
                a_ = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah_b, bhb[j], a_, 0, 0, 0);                                            \
                a_ = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(nb_cat8(al_a, al_b), nb_cat8(bla[j], blb[j]), a_, 0, 0, 0, sa, 0, sb); } }
#ifdef NB_ABL_NODMA       // developer ablation: no LDS-DMA inside the K loop (the chunks read what the prologue staged)
#define NB_DMA(slot) {}
#else
#define NB_DMA(slot) { if constexpr (DMA) { __builtin_amdgcn_sched_barrier(0); issue_at(std::integral_constant<int, slot>{}, S4{}, cn, sn); __builtin_amdgcn_sched_barrier(0); } }
#endif
            // Program order = issue order (a scheduling fence after every group): left to itself the scheduler sinks each
            // fragment read to just before its first use (register pressure), and every MFMA group then starts with an
            // exposed `s_waitcnt lgkmcnt(0)`.  With the reads of the NEXT group issued before the current group's MFMAs the
            // compiler's own wait bookkeeping emits counted waits (lgkmcnt(4), (2), (8), ...) and the reads return under
            // 256 cycles of matrix work.
#define NB_FENCE() __builtin_amdgcn_sched_barrier(0)
            // first group's operands in the order its MFMAs take them (the counted waits then release the first MFMA after
            // three reads, not after all sixteen), then the second group's A fragments
            NB_RD(a1h, st[aoff + 8 * 128]);
#pragma unroll
            for (int j = 0; j < NBE; ++j) NB_RD(b0h[j], st[boff[j]]);
            NB_RD(a2h, st[aoff + 6 * 128]);
#pragma unroll
            for (int j = 0; j < NBE; ++j) NB_RD(b1h[j], st[boff[j] + 1]);
            NB_RD(a1l, st[aoff + 8 * 128 + 32]); NB_RD(a2l, st[aoff + 6 * 128 + 32]);
#pragma unroll
            for (int j = 0; j < NBE; ++j) { NB_RD(b0l[j], st[boff[j] + XPL]); NB_RD(b1l[j], st[boff[j] + XPL + 1]); }
            NB_LDA(5, n1h, n1l); NB_LDA(3, n2h, n2l);                             // (for the second group)
            NB_FENCE();
            NB_PAIR(0, a1h, a1l, b0h, b0l, a2h, a2l, b1h, b1l);                   // taps 8, 6
            NB_FENCE();
            NB_DMA(0);
            NB_LDA(4, a1h, a1l);                                                  // (for the third group)
            NB_FENCE();
            NB_PAIR(2, n1h, n1l, b0h, b0l, n2h, n2l, b1h, b1l);                   // taps 5, 3
            NB_FENCE();
            NB_DMA(1);
            NB_LDB(XS, b1h, b1l); NB_LDA(7, n1h, n1l); NB_LDA(1, n2h, n2l);       // (for the fourth group)
            NB_FENCE();
#pragma unroll
            for (int j = 0; j < NBE; ++j) {                                       // tap 4 alone
                f32x16& a_ = acc[j][3];
                a_ = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1h, b0h[j], a_, 0, 0, 0);
                a_ = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(nb_cat8(a1l, z8), nb_cat8(b0l[j], z8), a_, 0, 0, 0, sa, 0, sb);
            }
            NB_FENCE();
            NB_DMA(2);
            NB_LDB(XS + 1, b2h, b2l); NB_LDA(2, a1h, a1l); NB_LDA(0, a2h, a2l);   // (for the fifth group)
            NB_FENCE();
            NB_PAIR(1, n1h, n1l, b0h, b0l, n2h, n2l, b1h, b1l);                   // taps 7, 1
            NB_FENCE();
            NB_DMA(3);
            NB_PAIR(0, a1h, a1l, b1h, b1l, a2h, a2l, b2h, b2l);                   // taps 2, 0
#undef NB_FENCE
#undef NB_LDA
#undef NB_LDB
#undef NB_PAIR
#undef NB_DMA
        } else {
            h8 ah[2], al[2], bh[2][NBJ], bl[2][NBJ];
            ah[0] = st[aoff + kOrd[0] * 128]; al[0] = st[aoff + kOrd[0] * 128 + 32];
#pragma unroll
            for (int j = 0; j < NBE; ++j) { bh[0][j] = st[boff[j] + kDel[0]]; bl[0][j] = st[boff[j] + XPL + kDel[0]]; }
            nb_static_for<0, 9>([&](auto ii) {
                constexpr int i = decltype(ii)::value;
                constexpr int ca = i & 1, cb = kGrp[i] & 1;
                constexpr int NBT = kPha[i] >= 2 ? NBE : NB01;            // blocks that take this tap
                constexpr int NBF = kGrp[i + 1 < 9 ? i + 1 : i] >= 2 ? NB01 : NBE;      // blocks that need the next offset group's B fragments (groups 2, 3 = taps 1, 2, 0: even-row phases only)
                f32x16& a0 = acc[0][kPha[i]];
                if constexpr (NBT > 0) a0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[ca], bh[cb][0], a0, 0, 0, 0);
                constexpr int nfetch = i + 1 < 9 ? (kGrp[i + 1 < 9 ? i + 1 : i] != kGrp[i] ? 2 + 2 * NBF : 2) : 0;
                if constexpr (i + 1 < 9) {
                    ah[ca ^ 1] = st[aoff + kOrd[i + 1] * 128]; al[ca ^ 1] = st[aoff + kOrd[i + 1] * 128 + 32];
                    if constexpr (kGrp[i + 1] != kGrp[i]) {
#pragma unroll
                        for (int j = 0; j < NBF; ++j) {
                            bh[cb ^ 1][j] = st[boff[j] + kDel[i + 1]]; bl[cb ^ 1][j] = st[boff[j] + XPL + kDel[i + 1]];
                        }
                    }
                }
                if constexpr (NBT > 0) {
                    a0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[ca], bl[cb][0], a0, 0, 0, 0);
                    a0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[ca], bh[cb][0], a0, 0, 0, 0);
                }
#pragma unroll
                for (int j = 1; j < NBT; ++j) {
                    f32x16& aj = acc[j][kPha[i]];
                    aj = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[ca], bh[cb][j], aj, 0, 0, 0);
                    aj = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[ca], bl[cb][j], aj, 0, 0, 0);
                    aj = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[ca], bh[cb][j], aj, 0, 0, 0);
                }
                // next tap's fragment reads go out BEFORE this tap's six MFMAs (their registers are free: the previous tap
                // has issued), which gives the LDS the whole tap to answer
                if constexpr (nfetch > 0) __builtin_amdgcn_sched_group_barrier(0x100, nfetch, 0);
                if constexpr (NBT > 0) __builtin_amdgcn_sched_group_barrier(0x008, 3 * NBT, 0);
                // this chunk's share of the next-but-one chunk's LDS-DMA pieces, behind the tap's MFMAs (taps 0..7)
                if constexpr (DMA && i < 8) {
                    __builtin_amdgcn_sched_barrier(0);
                    issue_at(ii, std::integral_constant<int, 8>{}, cn, sn);
                    __builtin_amdgcn_sched_barrier(0);
                }
            });
        }
        __builtin_amdgcn_sched_barrier(0);
    };
    auto kloop = [&](auto nbe) {
    int c = 0;
    int s_cur = 0;                                    // stage of chunk c
    if constexpr (NST == 2) {
        // two stages: chunk c+1 lands in the other stage while chunk c is multiplied; the wait at the end of a chunk is for
        // pieces issued during it -- exposed latency that the co-resident workgroup's matrix work covers
        for (; c + 1 < NC; ++c) {
            chunk(std::true_type{}, nbe, ring + s_cur * STAGE, c + 1, ring + (s_cur ^ 1) * STAGE);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            s_cur ^= 1;
        }
    }
    for (; NST == 3 && c + 2 < NC; ++c) {
        const int s_nn = s_cur == 0 ? 2 : s_cur - 1;  // (c + 2) % 3
        chunk(std::true_type{}, nbe, ring + s_cur * STAGE, c + 2, ring + s_nn * STAGE);
        // chunk c+1 has landed (the pieces of c+2 may stay in flight); everybody is done reading chunk c
        // (no timestamp reads in here: the branches around them split the loop body into several basic blocks, and the
        //  compiler then sinks MFMAs past the wait and the barrier)
#ifdef NB_ABL_NODMA
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#else
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NPC) : "memory");
#endif
#ifndef NB_ABL_NOBARRIER
        __builtin_amdgcn_s_barrier();
#endif
        s_cur = s_cur == 2 ? 0 : s_cur + 1;
    }
    for (; c < NC; ++c) {
        chunk(std::false_type{}, nbe, ring + s_cur * STAGE, 0, nullptr);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        s_cur = s_cur == NST - 1 ? 0 : s_cur + 1;
    }
    };
    // (copies of the loop per number of column blocks a wave really has to multiply: blocks that do not exist -- the 16th of the
    //  15-block tile -- or lie wholly below the image -- the last tile row of a height that 12 does not divide -- cost no MFMAs and
    //  no fragment reads; the DMA pieces and barriers are the same in every copy.  Their accumulators stay zero; nothing that is
    //  stored reads them.)
    const int nvalid_blk = (min(TQH, H - I0) + 2) * PW;                  // positions of the rows that feed stored pixels ...
    int nbe_w = 0;                                                       // ... and this wave's blocks that hold any of them
#pragma unroll
    for (int j = 0; j < NBJ; ++j) nbe_w += (wv + NW * j) * 32 < nvalid_blk && j < nblk;
    // the wave whose last multiplied block is the tile's last one, when that block holds nothing but the last halo row
    constexpr bool LASTROW_BLK = (NBLK - 1) * 32 >= (PH - 1) * PW;
    const bool half_last = LASTROW_BLK && !(p.dbg & 16) && wv == (NBLK - 1) % NW && nbe_w == (NBLK - 1) / NW + 1;
    if constexpr (NBJ > 1) {
        if (nbe_w == 2) { if (half_last) kloop(std::integral_constant<int, 2 | 4>{}); else kloop(std::integral_constant<int, 2>{}); }
        else if (nbe_w == 1) { if (half_last) kloop(std::integral_constant<int, 1 | 4>{}); else kloop(std::integral_constant<int, 1>{}); }
        else kloop(std::integral_constant<int, 0>{});
    } else {
        if (nbe_w == 1) { if (half_last) kloop(std::integral_constant<int, 1 | 4>{}); else kloop(std::integral_constant<int, 1>{}); }
        else kloop(std::integral_constant<int, 0>{});
    }
    if (p.tstamps && tid == 0) {
        unsigned long long* ts = p.tstamps + (size_t)(blockIdx.x + blockIdx.y * gridDim.x) * 8;
        ts[6] = t_dma; ts[7] = t_bar | ((__builtin_amdgcn_s_memtime() - t_loop0) << 32);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");              // drain before the staging LDS is reused
    __builtin_amdgcn_s_barrier();

    NB_TSTAMP(2);
    if (p.dbg & 4) { if (acc[0][0][0] == 123.456f) p.y[0] = 0.f; return; }      // ablation: main loop only
    // ---- epilogue: 2 rounds of 16 c_out.  Accumulator register rho <-> c_out row (rho&3) + 8(rho>>2) + 4*lh, so the four
    //      registers rho = 4g..4g+3 of a lane are four CONSECUTIVE channels: they go to LDS as one 16-byte slot
    //      y4[g&1][lh][phase][position].  Then one item = one quad (2 x 2 output pixels) x those 4 channels: 25 slot reads,
    //      the separable polyphase FIR with every instruction packed over channel pairs (no lane-half shuffles), activation,
    //      hi/lo split and fp8 conversion in registers.  Lanes l and l+32 hold the two channel halves of the same quad and
    //      trade rows with v_permlane32_swap, after which a lane owns 8 channels of one output row of the quad = whole
    //      16-byte H2 slots (8-byte halves of the f8 slots) that go straight to global memory: no staging buffer, no
    //      transposition stage, 4 barriers instead of 12. ----
    const int Wo = 2 * W, Ho = 2 * H;
    constexpr int nquads = TQH * TQW;
    constexpr int Y1P = NBLK * 32;                    // slots per (g, lh, phase) plane
    f32x4* y4 = reinterpret_cast<f32x4*>(smem_h3);
    const float clampv = p.clamp >= 0.f ? p.clamp : __builtin_inff();     // (no clamp: med3 against +-inf)
    unsigned long long te_w = 0, te_f = 0, te0 = 0;   // debug: cycles in (phase write + sync), (items)
#pragma unroll
    for (int R = 0; R < 2; ++R) {
        if (p.tstamps) te0 = __builtin_amdgcn_s_memtime();
        // LDS-only barriers: __syncthreads() would also wait (vmcnt(0)) for the previous round's global stores to retire
        if (R) asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");     // the previous round's reads are done
#pragma unroll
        for (int gs = 0; gs < 2; ++gs) {
            const int r0 = (2 * R + gs) * 4;
#pragma unroll
            for (int j = 0; j < NBJ; ++j) {
                if (j < nblk) {
                    const int pidx = (wv + NW * j) * 32 + l31;
#pragma unroll
                    for (int ph = 0; ph < 4; ++ph)
                        y4[((gs * 2 + lh) * 4 + ph) * Y1P + pidx] = f32x4{acc[j][ph][r0], acc[j][ph][r0 + 1], acc[j][ph][r0 + 2], acc[j][ph][r0 + 3]};
                }
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        if (p.tstamps) { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); te_w += t_ - te0; te0 = t_; }
        auto quad_item = [&](const int wi) {
            const int hq = wi * 32 + l31;             // (g, quad); lane half = channel half
            const int gs = hq / nquads, qd = hq - gs * nquads;
            const int ti = qd / TQW, tj = qd - ti * TQW;
            if (I0 + ti >= H) return;                 // quad row below the image (ragged last tile row): nothing of it is stored
            const int c4 = 8 * (2 * R + gs) + 4 * lh; // the lane's four channels within the slice
            const f32x4* ee = y4 + ((gs * 2 + lh) * 4) * Y1P + ti * PW + tj;
            const f32x4* eo = ee + 1 * Y1P;
            const f32x4* oe = ee + 2 * Y1P;
            const f32x4* oo = ee + 3 * Y1P;
            // horizontal pass first (nb_up2_hrow, nb_h3_common.h): the quad's five pre-filter rows O(ti), E(ti), O(ti + 1), E(ti + 1),
            // O(ti + 2) at its two output columns; then one vertical FIR per output row (nb_up2_vout) -- the per-output order of
            // modconv3x3_up2v_kernel, which shares the filtered rows along a column run of quads
            f32x4 hr[5][2];
#pragma unroll
            for (int m = 0; m < 5; ++m) {
                if (m & 1) nb_up2_hrow(ee + (m >> 1) * PW, eo + (m >> 1) * PW, hr[m]);
                else nb_up2_hrow(oe + (m >> 1) * PW, oo + (m >> 1) * PW, hr[m]);
            }
            const f32x4 d4 = *reinterpret_cast<const f32x4*>(s_dco + c4), b4 = *reinterpret_cast<const f32x4*>(s_bias + c4);
            const int qi = I0 + ti, qj = J0 + tj;
            f32x4 v[2][2];                            // [dy][px]
#pragma unroll
            for (int dy = 0; dy < 2; ++dy) {
                const f32x2 nz = *reinterpret_cast<const f32x2*>(s_noise + (2 * ti + dy) * (2 * TQW) + 2 * tj);
                // The two noise values get registers of their own.  Left in the loaded pair, the compiler adds the second one
                // as `v_pk_add_f32 d, bias, v[pair] op_sel:[0,1]` (low result reads the pair's HIGH dword), and that
                // instruction returned, for 8-16 lanes of the upper half-wave and run-to-run differently, the sum with the
                // pair's LOW dword in its low result (measured: tools/determinism_up2.py; waits forced to zero and s_nops
                // did not change it, this did).
                float nz0 = nz[0], nz1 = nz[1];
                asm volatile("v_mov_b32 %0, %0" : "+v"(nz0));
                asm volatile("v_mov_b32 %0, %0" : "+v"(nz1));
                nb_up2_vout(hr[dy], hr[dy + 1], hr[dy + 2], hr[dy + 3], d4, b4, nz0, nz1, p.alpha, clampv, v[dy]);
            }
            if constexpr (OUTM == 0) {
                if (qi < H && !(p.dbg & 1)) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int co = co0 + c4 + i;
                        if (co < p.c_out) {
                            float* dst = p.y + ((size_t)n * p.c_out + co) * ((size_t)Ho * Wo) + (size_t)(2 * qi) * Wo + 2 * qj;
                            *reinterpret_cast<f32x2*>(dst) = f32x2{v[0][0][i], v[0][1][i]};
                            *reinterpret_cast<f32x2*>(dst + Wo) = f32x2{v[1][0][i], v[1][1][i]};
                        }
                    }
                }
            } else {
                const f32x4 ns4 = *reinterpret_cast<const f32x4*>(s_nst + c4);
                unsigned hi[2][2][2], lo[2][2][2];    // [dy][px][dword]: hi = 4 x f16; lo = H2: 4 x f16 residual, f8: {fp8(xl 2^9) x 4, fp8(v/4) x 4}
#pragma unroll
                for (int dy = 0; dy < 2; ++dy)
#pragma unroll
                    for (int px = 0; px < 2; ++px) {
                        f32x4 w = v[dy][px] * ns4;
                        const h2 h01 = __builtin_convertvector(f32x2{w[0], w[1]}, h2), h23 = __builtin_convertvector(f32x2{w[2], w[3]}, h2);
                        // residual w - f16(w) as a mixed-precision fma (reads the f16 half directly)
                        const f32x4 xl = {nb_sub_f16(w[0], h01, false), nb_sub_f16(w[1], h01, true), nb_sub_f16(w[2], h23, false), nb_sub_f16(w[3], h23, true)};
                        hi[dy][px][0] = __builtin_bit_cast(unsigned, h01); hi[dy][px][1] = __builtin_bit_cast(unsigned, h23);
                        if constexpr (OUTM == 1) {
                            const h2 l01 = __builtin_convertvector(f32x2{xl[0], xl[1]}, h2), l23 = __builtin_convertvector(f32x2{xl[2], xl[3]}, h2);
                            lo[dy][px][0] = __builtin_bit_cast(unsigned, l01); lo[dy][px][1] = __builtin_bit_cast(unsigned, l23);
                        } else {
                            // (conversions saturate: FP16_OVFL is set for this kernel)
                            // (x 2^9 and x 2^-2 inside the conversions: nb_pk4_fp8_sat_scaled)
                            lo[dy][px][0] = nb_pk4_fp8_sat_scaled(xl[0], xl[1], xl[2], xl[3], 0x1p-9f);
                            lo[dy][px][1] = nb_pk4_fp8_sat_scaled(w[0], w[1], w[2], w[3], 4.f);
                        }
                    }
                // lanes l (channels 0-3 of the group) and l+32 (channels 4-7) trade rows: afterwards a lane holds output row
                // dy = lh of the quad with all 8 channels -- a = channels 0-3, b = channels 4-7
                unsigned ha[2][2], hb[2][2], la[2][2], lb[2][2];     // [px][dword]
#pragma unroll
                for (int px = 0; px < 2; ++px)
#pragma unroll
                    for (int k = 0; k < 2; ++k) {
                        ha[px][k] = hi[0][px][k]; hb[px][k] = hi[1][px][k]; la[px][k] = lo[0][px][k]; lb[px][k] = lo[1][px][k];
                        nb_swap32(ha[px][k], hb[px][k]);
                        nb_swap32(la[px][k], lb[px][k]);
                    }
                const int cg = co0 / 8 + 2 * R + gs;
                const int oy = 2 * qi + lh, ox = 2 * qj;
                if (qi < H && cg * 8 < p.c_out && !(p.dbg & 1)) {
                    const size_t OHW8 = (size_t)Ho * Wo * 8;
                    _Float16* yn = p.yh2 + ((size_t)n * p.c8_next + cg) * 2 * OHW8;
                    const size_t opix8 = ((size_t)oy * Wo + ox) * 8;
#pragma unroll
                    for (int px = 0; px < 2; ++px) {
                        *reinterpret_cast<u32x4*>(yn + opix8 + px * 8) = u32x4{ha[px][0], ha[px][1], hb[px][0], hb[px][1]};
                        if constexpr (OUTM == 1) {
                            *reinterpret_cast<u32x4*>(yn + OHW8 + opix8 + px * 8) = u32x4{la[px][0], la[px][1], lb[px][0], lb[px][1]};
                        } else {
                            // the 16-channel chunk's two lo slots: (even group, lo) = fp8(xl 2^9) of its 16 channels, (odd group,
                            // lo) = fp8(v/4); this group's 8 channels are bytes 8 (cg & 1) .. + 7 of both
                            _Float16* lo_xl = p.yh2 + ((size_t)n * p.c8_next + (cg & ~1)) * 2 * OHW8 + OHW8 + opix8 + px * 8 + (cg & 1) * 4;
                            *reinterpret_cast<u32x2*>(lo_xl) = u32x2{la[px][0], lb[px][0]};
                            *reinterpret_cast<u32x2*>(lo_xl + 2 * OHW8) = u32x2{la[px][1], lb[px][1]};
                        }
                    }
                }
            }
        };
        constexpr int NWI = nquads * 2 / 32;          // wave-iterations of 32 quads x both channel halves per round
        static_assert(nquads * 2 % 32 == 0, "tile quads must fill whole waves");
        if constexpr (NWI % NW == 0) {
#pragma unroll
            for (int k = 0; k < NWI / NW; ++k) quad_item(wv + k * NW);
        } else {
            for (int wi = wv; wi < NWI; wi += NW) quad_item(wi);
        }
        if (p.tstamps) { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); te_f += t_ - te0; }
    }
    const unsigned long long te_s = 0;
    NB_TSTAMP(4);
    if (p.tstamps) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        NB_TSTAMP(5);
        if (threadIdx.x == 0) p.tstamps[(size_t)(blockIdx.x + blockIdx.y * gridDim.x) * 8 + 3] = (te_w & 0x1fffff) | ((te_f & 0x1fffff) << 21) | ((te_s & 0x1fffff) << 42);
    }
}

static int g_force_tqh = -1;
// developer / test hook: 0 = automatic tile choice, NB_H3_TQH, NB_H3_TQH_MID or NB_H3_TQH_SMALL = force that tile height
extern "C" void nb_debug_set_up2_tile(int tqh) { g_force_tqh = tqh; }
// the 8-wave form with the software-pipelined K loop (nb_modconv_up2v.hip)
bool nb_up2v_eligible(int in_fmt, int c_in, int h, int w);
int nb_up2v_launch(H3Up2Params p, int n, int in_fmt, void* stream, unsigned long long* tstamps, int tstamps_cap, bool auto_rows);
#ifndef NB_UP2V_AUTO
#define NB_UP2V_AUTO 1          // 1: f8 launches on the 12-row throughput tiles run on the software-pipelined kernel
#endif
static int g_force_v2 = -1;
// developer / test hook: -1 = automatic, 0 = never, 1 = wherever the shape allows (f8 operands, w % 32 == 0; always 12-row tiles)
extern "C" void nb_debug_set_up2_v2(int mode) { g_force_v2 = mode; }
static int g_force_pair = -1;
// developer / test hook: -1 = automatic, 0 / 1 = never / always the two-workgroups-per-CU form (4 waves, 12 x 16 tiles, 2 stages)
extern "C" void nb_debug_set_up2_pair(int mode) { g_force_pair = mode; }
template <int TQH, int TQW, bool F8, int OUTM, int NW, int NST>
static int nb_up2_h3_launch1(const H3Up2Params& p, int n, size_t lds, void* stream) {
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute((const void*)modconv3x3_up2_h3_kernel<F8, TQH, OUTM, TQW, NW, NST>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        attr_set = true;
    }
    dim3 grid(p.tiles_x * p.tiles_y * p.slices, n);
    hipLaunchKernelGGL((modconv3x3_up2_h3_kernel<F8, TQH, OUTM, TQW, NW, NST>), grid, dim3(NW * 64), lds, (hipStream_t)stream, p);
    NB_CHECK_LAUNCH("modconv3x3_up2_h3");
    return NB_OK;
}

template <int TQH, int TQW = 32, int NW = 8, int NST = NB_H3_STAGES>
static int nb_up2_h3_launch(H3Up2Params p, int n, int in_fmt, void* stream) {
    p.tiles_x = p.w / TQW;
    p.tiles_y = (p.h + TQH - 1) / TQH;
    p.tstamps = (g_tstamps && (long long)p.tiles_x * p.tiles_y * p.slices * n <= g_tstamps_cap) ? g_tstamps : nullptr;
    constexpr int XPL = (TQH + 3) * (TQW + 3);
    constexpr int NBLK_ = ((TQH + 2) * (TQW + 2) + 31) / 32;
    constexpr size_t lds_stage = (size_t)NST * (4 * XPL + 36 * 32) * 16;
    static_assert(NBLK_ <= 2 * NW, "two column blocks per wave at most");
    constexpr size_t lds_epi = (size_t)16 * NBLK_ * 32 * 16;       // epilogue: [2 groups][2 halves][4 phases][positions] x 4 channels fp32
    const size_t lds = lds_stage > lds_epi ? lds_stage : lds_epi;
    const int outm = p.yh2 ? (p.out_f8 ? 2 : 1) : 0;
    auto go = [&](auto f8_) {
        constexpr bool F8_ = decltype(f8_)::value;
        return outm == 2 ? nb_up2_h3_launch1<TQH, TQW, F8_, 2, NW, NST>(p, n, lds, stream) : outm == 1 ? nb_up2_h3_launch1<TQH, TQW, F8_, 1, NW, NST>(p, n, lds, stream)
                                                                                             : nb_up2_h3_launch1<TQH, TQW, F8_, 0, NW, NST>(p, n, lds, stream);
    };
    if constexpr (NW == 4) {      // the two-per-CU form exists for H2 operands only (its f8 form spills 1-3 registers: not with counted waits)
        NB_REQUIRE(!in_fmt, "modconv3x3_up2_h3: the two-workgroups-per-CU form takes H2 operands only");
        return go(std::false_type{});
    } else
    return in_fmt ? go(std::true_type{}) : go(std::false_type{});
}

// which kernel a split-f16 up=2 launch runs on (the debug hooks apply)
enum Up2Form { UP2_BIG = 0, UP2_MID, UP2_SMALL, UP2_W16, UP2_PAIR, UP2_V2, UP2_W8 };
static Up2Form nb_up2_h3_select(int in_fmt, int c_in, int c_out, int n, int h, int w) {
    const int tiles_x = w / 32, slices = (c_out + 31) / 32;
    if (w == 16) return UP2_W16;                      // 16-wide inputs: 8 x 16 quad tiles
    if (w == 8) return UP2_W8;                        // 8 x 8 inputs: the whole image is one 8 x 8 quad tile (4 position blocks)
    // tile height: the 12-row tiles unless they leave the chip mostly idle (batch-1 / interactive), then 5-row tiles
    const int force_tqh = g_force_tqh >= 0 ? g_force_tqh : 0;
    const long wgs_big = (long)n * tiles_x * ((h + NB_H3_TQH - 1) / NB_H3_TQH) * slices;
    const bool small_tiles = force_tqh ? force_tqh == NB_H3_TQH_SMALL : wgs_big < 160;
    // 8-row tiles when the 12-row tiles' last round of workgroups would leave most of the chip idle.  Estimate = rounds of 256
    // workgroups x cost of one (critical SIMD's position blocks 4 / 3, + prologue and epilogue ~ quads): b64.conv0 at batch 32
    // (32 input rows) is 384 workgroups = 1.5 rounds of 12-row tiles, but 512 = 2 full rounds of 8-row tiles at 0.73 the cost.
    bool mid_tiles = force_tqh == NB_H3_TQH_MID;
    if (!force_tqh && !small_tiles) {
        constexpr long ncu = 256;                     // MI355X (one workgroup of this kernel per CU)
        const long wgs_mid = (long)n * tiles_x * ((h + NB_H3_TQH_MID - 1) / NB_H3_TQH_MID) * slices;
        const double est_big = (double)((wgs_big + ncu - 1) / ncu) * 5.4, est_mid = (double)((wgs_mid + ncu - 1) / ncu) * 3.93;
        mid_tiles = est_mid < 0.9 * est_big;
    }
    // two 4-wave workgroups per CU on 12 x 16 tiles (see the kernel's NW_ / NST_) when that launch fills the chip as well
    const bool pair = !in_fmt && g_force_pair > 0;          // (opt-in through nb_debug_set_up2_pair: not faster than one 8-wave workgroup per CU)
    if (pair) return UP2_PAIR;
    // the 12-row throughput tiles of an f8 launch: the kernel with the software-pipelined K loop (same tile, same results)
    const int force_v2 = g_force_v2;
    if (force_v2 != 0 && nb_up2v_eligible(in_fmt, c_in, h, w) &&
        (force_v2 > 0 ? force_tqh == 0 || force_tqh == NB_H3_TQH : (NB_UP2V_AUTO && !mid_tiles && !small_tiles && (force_tqh == 0 || force_tqh == NB_H3_TQH))))
        return UP2_V2;
    if (mid_tiles) return UP2_MID;
    return small_tiles ? UP2_SMALL : UP2_BIG;
}

static int nb_up2_h3_impl(const H3ConvArgs& a, void* stream, int in_fmt = 0) {
    const int n = a.n, h = a.h, w = a.w, c_in = a.c_in, c_out = a.c_out, out_fmt = a.out_fmt;
    NB_REQUIRE(in_fmt >= 0 && in_fmt <= 3 && (out_fmt == 0 || out_fmt == 1), "modconv3x3_up2_h3: input operand format must be 0 (H2), 1 (f8), 2 (f6) or 3 (f8, hi only), "
               "output format 0 or 1 (the up=2 epilogue does not write the f6 format)");
    NB_REQUIRE(in_fmt == 0 || c_in % 16 == 0, "modconv3x3_up2_h3: the f8 / f6 operand formats need c_in %% 16 == 0 (got %d)", c_in);
    NB_REQUIRE(out_fmt == 0 || (a.y_h2 && c_out % 16 == 0 && a.c_next % 16 == 0), "modconv3x3_up2_h3: f8 output needs an H2 destination and c_out, c_next %% 16 == 0");
    NB_REQUIRE(a.x_h2 && a.w_h3 && a.dcoefs && a.bias && ((a.y != nullptr) != (a.y_h2 != nullptr)), "modconv3x3_up2_h3: null pointer");
    H3Up2Params p;
    if (const int rc = nb_h3_launch_setup(p, "modconv3x3_up2_h3", a, 2, (w % 32 == 0 || w == 16 || w == 8) && h >= 8, "w % 32 == 0, w == 16 or w == 8", false)) return rc;
    p.tiles_x = w / 32; p.slices = (c_out + 31) / 32;
    const Up2Form form = nb_up2_h3_select(in_fmt, c_in, c_out, n, h, w);
    NB_REQUIRE(in_fmt != 2 || form == UP2_V2, "modconv3x3_up2_h3: f6 operands are taken by the 12-row software-pipelined kernel only (this launch: %dx%d, batch %d)", h, w, n);
    switch (form) {
        case UP2_W16: return nb_up2_h3_launch<8, 16>(p, n, in_fmt, stream);
        case UP2_W8: return nb_up2_h3_launch<8, 8>(p, n, in_fmt, stream);
        case UP2_PAIR: return nb_up2_h3_launch<NB_H3_TQH, 16, 4, 2>(p, n, in_fmt, stream);
        case UP2_V2: return nb_up2v_launch(p, n, in_fmt, stream, g_tstamps, g_tstamps_cap, g_force_v2 < 0);      // (forced: 12-row tiles)
        case UP2_MID: return nb_up2_h3_launch<NB_H3_TQH_MID>(p, n, in_fmt, stream);
        case UP2_SMALL: return nb_up2_h3_launch<NB_H3_TQH_SMALL>(p, n, in_fmt, stream);
        default: return nb_up2_h3_launch<NB_H3_TQH>(p, n, in_fmt, stream);
    }
}

extern "C" int nb_modconv3x3_up2_h3_variant(int in_fmt, int c_in, int c_out, int n, int h, int w, char* buf, int buflen) {
    NB_REQUIRE(buf && buflen > 0, "modconv3x3_up2_h3_variant: bad buffer");
    NB_REQUIRE(in_fmt >= 0 && in_fmt <= 3 && n > 0 && c_in > 0 && c_out > 0 && h >= 8 && (w % 32 == 0 || w == 16 || w == 8), "modconv3x3_up2_h3_variant: bad shape");
    snprintf(buf, buflen, "%s", nb_up2_h3_select(in_fmt, c_in, c_out, n, h, w) == UP2_V2 ? "modconv3x3_up2v_kernel" : "modconv3x3_up2_h3_kernel");
    return NB_OK;
}

extern "C" int nb_modconv3x3_up2_h3(const void* x_h2, int c_in, const void* w_h3, const float* dcoefs, const float* noise,
                                    int64_t noise_stride_n, const float* bias, float* y, int n, int h, int w, int c_out,
                                    float alpha, float gain, float clamp, void* stream) {
    return nb_up2_h3_impl({x_h2, c_in, w_h3, dcoefs, noise, noise_stride_n, bias, y, nullptr, nullptr, 0, 0, n, h, w, c_out, alpha, gain, clamp, 0}, stream);
}

extern "C" int nb_modconv3x3_up2_h3_ex(const void* x, int c_in, const void* wts, const float* dcoefs, const float* noise,
                                      int64_t noise_stride_n, const float* bias, float* y_f32, void* y_h2,
                                      const float* next_styles, int next_stride, int c_next, int in_fmt, int out_fmt, int n,
                                      int h, int w, int c_out, float alpha, float gain, float clamp, void* stream) {
    return nb_up2_h3_impl({x, c_in, wts, dcoefs, noise, noise_stride_n, bias, y_f32, y_h2, next_styles, next_stride, c_next, n, h, w, c_out, alpha, gain, clamp, out_fmt}, stream, in_fmt);
}

extern "C" int nb_modconv3x3_up2_h3_h2(const void* x_h2, int c_in, const void* w_h3, const float* dcoefs, const float* noise,
                                       int64_t noise_stride_n, const float* bias, const float* next_styles, int next_stride,
                                       void* y_h2, int c_next, int n, int h, int w, int c_out, float alpha, float gain,
                                       float clamp, void* stream) {
    return nb_up2_h3_impl({x_h2, c_in, w_h3, dcoefs, noise, noise_stride_n, bias, nullptr, y_h2, next_styles, next_stride, c_next, n, h, w, c_out, alpha, gain, clamp, 0}, stream);
}
