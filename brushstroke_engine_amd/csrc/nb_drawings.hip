// Synthetic stroke drawings on the device for gfx950: seeded random centripetal Catmull-Rom patches, K at a time -- what the
// reference's scripts/create_splines.py makes one image per process-pool task on the host.  Three entries (include/neube_hip.h states
// the draws):
//   nb_synth_spline_counts     control points per drawing (HOST ONLY: integer arithmetic on one Philox call per drawing)
//   nb_synth_spline_ctrl_f32   the packed control points (x, y, r_eff) of K drawings: the sampler of forger/core/curve.py:98-116
//                              (sample_control_pts2) and scripts/create_splines.py:35-39, the thickness of forger/util/spline_dist.py
//   nb_raster_batch_u8         K drawings' segment rows -> [K,h,w] uint8 in one launch, each drawing under the contract of
//                              nb_raster_segments_u8 with clear = 1 and bit-identical to it (the per-cell code is shared:
//                              nb_raster_cell.h)
// Between the two device entries runs nb_spline_flatten_f32 (csrc/nb_strokes.hip) as it is.
//
// fp32 roundings of a coordinate (the bound of tests/test_hip_drawings.py is NB_SYNTH_COORD_ROUNDINGS * ulp(1.1 r)): u = (x >> 8) *
// 2^-24 and r / 4 are exact;
//   cells, i < 16     (c + u) * (r / 4)            2 roundings: the sum, the product
//   cells, i >= 16    (u * 1.1f - 0.05f) * r       3 roundings: product, difference, product
//   uniform           (u * 1.1f) * r               2 roundings
// with 1.1f and 0.05f the fp32 constants (the float64 restatement uses the same two values).  Each rounding is at most half an ulp of
// a value that, scaled to pixels, is below 1.1 r; the scaling by an r that is no power of two can double it: one ulp(1.1 r) per
// rounding, three at the most.
// Scalar fp32, unfused (-ffp-contract=off), no SLP pairing (build.py FILE_FLAGS), as csrc/nb_strokes.hip.
#include "nb_common.h"
#include "nb_philox.h"
#include "nb_raster_cell.h"
#include <cstdint>
#include <cmath>

namespace {

constexpr uint32_t SPLN = 0x53504C4Eu;     // counter word 1 of every draw of a drawing ("SPLN")
constexpr int TRIES = 8;                   // Gaussian thickness tries: draws P(1) .. P(8)
constexpr int CTRL_DRAW0 = 16;             // control point i is draw P(16 + i)

__host__ __device__ __forceinline__ void draw(uint32_t j, uint64_t s, uint64_t seed, uint32_t x[4]) {
    nb_philox4x32_10(j, SPLN, (uint32_t)s, (uint32_t)(s >> 32), (uint32_t)seed, (uint32_t)(seed >> 32), x);
}

__host__ __device__ __forceinline__ int points_of(const NbSplineSpec& sp, uint32_t x0) {
    return sp.pts_min + (int)(x0 % (uint32_t)(sp.pts_max - sp.pts_min + 1));
}

__device__ __forceinline__ float unit_f(uint32_t x) { return (float)(x >> 8) * 0x1p-24f; }

// One lane per drawing: the choice of cells is sequential (without replacement), at most pts_max <= 64 steps.  The lane derives its
// own point count from P(0) and writes only if stroke_off agrees with it and stays inside ctrl.
__global__ __launch_bounds__(64) void synth_ctrl_kernel(NbSplineSpec sp, uint64_t seed, uint64_t offset, int k, int r,
                                                        const int32_t* __restrict__ stroke_off, float* __restrict__ ctrl,
                                                        int n_points_total) {
    const int d = (int)blockIdx.x * 64 + (int)threadIdx.x;
    if (d >= k) return;
    const uint64_t s = offset + (uint64_t)d;
    uint32_t x[4];
    draw(0u, s, seed, x);
    const int npts = points_of(sp, x[0]);
    const long long p0 = stroke_off[d], p1 = stroke_off[d + 1];
    if (p0 < 0 || p1 > n_points_total || p1 - p0 != npts) return;       // a table that disagrees with the counts: nothing written

    float radius = 0.f;
    if (sp.thick_mode == NB_THICK_FIXED) {
        radius = sp.radius;
    } else if (sp.thick_mode == NB_THICK_RANGE) {
        radius = (float)(sp.rmin + (int)(x[2] % (uint32_t)(sp.rmax - sp.rmin + 1)));
    } else {
        const float uc = unit_f(x[1]);
        int c = sp.n_mix - 1;
        for (int m = sp.n_mix - 2; m >= 0; --m)
            if (uc < sp.cdf[m]) c = m;                                  // the first component with u < cdf
        const float center = c == 0 ? sp.center[0] : c == 1 ? sp.center[1] : c == 2 ? sp.center[2] : sp.center[3];
        const float sigma = c == 0 ? sp.sigma[0] : c == 1 ? sp.sigma[1] : c == 2 ? sp.sigma[2] : sp.sigma[3];
        for (int i = 0; i < TRIES; ++i) {
            uint32_t t[4];
            draw(1u + (uint32_t)i, s, seed, t);
            float z, z_odd;
            nb_normal_pair(t[0], t[1], z, z_odd);
            const float v = center + sigma * z;
            if (v >= -0.5f) {
                radius = rintf(v);
                break;
            }
        }
    }
    const float r_eff = radius >= 2.f ? radius : 0.5f;

    const float fr = (float)r, quarter = fr * 0.25f;
    unsigned used = 0;                                                  // bit c: cell c of the 4 x 4 grid is taken
    float* out = ctrl + (size_t)p0 * 3;
    for (int i = 0; i < npts; ++i) {
        uint32_t t[4];
        draw((uint32_t)(CTRL_DRAW0 + i), s, seed, t);
        const float ux = unit_f(t[1]), uy = unit_f(t[2]);
        float px, py;
        if (sp.mode == NB_SPLINE_CELLS && i < 16) {
            int skip = (int)(t[0] % (uint32_t)(16 - i)), cell = 0;
            for (; cell < 15; ++cell) {                                 // the skip-th free cell in ascending index (skip < 16 - i free ones)
                if (used & (1u << cell)) continue;
                if (skip-- == 0) break;
            }
            used |= 1u << cell;
            px = ((float)(cell & 3) + ux) * quarter;
            py = ((float)(cell >> 2) + uy) * quarter;
        } else if (sp.mode == NB_SPLINE_CELLS) {
            px = (ux * 1.1f - 0.05f) * fr;
            py = (uy * 1.1f - 0.05f) * fr;
        } else {
            px = (ux * 1.1f) * fr;
            py = (uy * 1.1f) * fr;
        }
        out[3 * i + 0] = px;
        out[3 * i + 1] = py;
        out[3 * i + 2] = r_eff;
    }
}

// One 256-thread workgroup per 64 x 64 cell of one drawing: block b is cell b % ncells of drawing b / ncells.  The drawing's range
// of rows is read from seg_off and checked against the total before anything is addressed through it; a bad range is an empty one
// (the cell is filled with 255).  The rest is nb_raster_cell on that drawing's rows and that drawing's plane: a row darkens the
// plane of its own drawing only, clipped at the plane's edges by the cell's own bounds.
__global__ __launch_bounds__(256) void raster_batch_kernel(const float* __restrict__ segs, const int32_t* __restrict__ seg_off,
                                                           int n_segs_total, uint8_t* __restrict__ out, int h, int w, int off_y,
                                                           int off_x, int ncx, int ncells) {
    const int d = (int)(blockIdx.x / (unsigned)ncells), cell = (int)(blockIdx.x % (unsigned)ncells);
    const int cy0 = (cell / ncx) * NB_RASTER_CELL, cx0 = (cell % ncx) * NB_RASTER_CELL;
    long long a = seg_off[d], b = seg_off[d + 1];
    if (a < 0 || b > n_segs_total || b < a) a = b = 0;
    nb_raster_cell(segs + (size_t)a * NB_RASTER_SEG_PITCH, (unsigned)(b - a), out + (size_t)d * h * w, h, w, off_y, off_x, cy0, cx0, 1);
}

bool finite_host(float v) { return std::isfinite(v); }

int check_spec(const NbSplineSpec* sp, const char* what) {
    NB_REQUIRE(sp, "%s: null spec", what);
    NB_REQUIRE(sp->pts_min >= 4 && sp->pts_min <= sp->pts_max && sp->pts_max <= NB_SYNTH_MAX_POINTS,
               "%s: points %d..%d outside 4 <= min <= max <= %d", what, sp->pts_min, sp->pts_max, NB_SYNTH_MAX_POINTS);
    NB_REQUIRE(sp->mode == NB_SPLINE_UNIFORM || sp->mode == NB_SPLINE_CELLS, "%s: unknown sampling mode %d", what, sp->mode);
    if (sp->thick_mode == NB_THICK_FIXED) {
        NB_REQUIRE(finite_host(sp->radius) && sp->radius >= 0.f, "%s: fixed radius %g", what, (double)sp->radius);
    } else if (sp->thick_mode == NB_THICK_RANGE) {
        NB_REQUIRE(sp->rmin >= 0 && sp->rmin <= sp->rmax && sp->rmax <= (1 << 20), "%s: radius range %d..%d", what, sp->rmin, sp->rmax);
    } else if (sp->thick_mode == NB_THICK_MIXTURE) {
        NB_REQUIRE(sp->n_mix >= 1 && sp->n_mix <= NB_SYNTH_MAX_MIX, "%s: %d mixture components (1..%d)", what, sp->n_mix, NB_SYNTH_MAX_MIX);
        float prev = 0.f;
        for (int c = 0; c < sp->n_mix; ++c) {
            NB_REQUIRE(finite_host(sp->center[c]) && finite_host(sp->sigma[c]) && sp->sigma[c] >= 0.f,
                       "%s: mixture component %d: centre %g, sigma %g", what, c, (double)sp->center[c], (double)sp->sigma[c]);
            NB_REQUIRE(sp->cdf[c] >= prev && sp->cdf[c] <= 1.f, "%s: cdf[%d] = %g is not a cumulative weight", what, c, (double)sp->cdf[c]);
            prev = sp->cdf[c];
        }
        NB_REQUIRE(sp->cdf[sp->n_mix - 1] == 1.f, "%s: the last cdf entry must be 1, got %g", what, (double)sp->cdf[sp->n_mix - 1]);
    } else {
        NB_REQUIRE(false, "%s: unknown thickness mode %d", what, sp->thick_mode);
    }
    return NB_OK;
}

}  // namespace

extern "C" int nb_synth_spline_counts(const NbSplineSpec* spec, uint64_t seed, uint64_t offset, int k, int32_t* npts) {
    if (int rc = check_spec(spec, "synth_spline_counts")) return rc;
    NB_REQUIRE(k >= 0 && (npts || k == 0), "synth_spline_counts: %d drawings at a null pointer", k);
    for (int d = 0; d < k; ++d) {
        uint32_t x[4];
        draw(0u, offset + (uint64_t)d, seed, x);
        npts[d] = points_of(*spec, x[0]);
    }
    return NB_OK;
}

extern "C" int nb_synth_spline_ctrl_f32(const NbSplineSpec* spec, uint64_t seed, uint64_t offset, int k, int r, const int32_t* stroke_off,
                                        float* ctrl, int n_points_total, void* stream) {
    if (int rc = check_spec(spec, "synth_spline_ctrl")) return rc;
    NB_REQUIRE(stroke_off && ctrl, "synth_spline_ctrl: null pointer");
    NB_REQUIRE(k >= 1 && r >= 1 && r <= (1 << 20), "synth_spline_ctrl: %d drawings of side %d", k, r);
    NB_REQUIRE((long long)n_points_total >= (long long)spec->pts_min * k && (long long)n_points_total <= (long long)spec->pts_max * k,
               "synth_spline_ctrl: %d points in %d drawings of %d..%d", n_points_total, k, spec->pts_min, spec->pts_max);
    hipLaunchKernelGGL(synth_ctrl_kernel, dim3((unsigned)nb_cdiv(k, 64)), dim3(64), 0, (hipStream_t)stream, *spec, seed, offset, k, r,
                       stroke_off, ctrl, n_points_total);
    NB_CHECK_LAUNCH("synth_spline_ctrl");
    return NB_OK;
}

extern "C" int nb_raster_batch_u8(const float* segs, const int32_t* seg_off, int n_segs_total, int k, uint8_t* out, int h, int w,
                                  int off_y, int off_x, void* stream) {
    NB_REQUIRE(out && seg_off, "raster_batch: null pointer");
    NB_REQUIRE(n_segs_total >= 0 && (segs || n_segs_total == 0), "raster_batch: %d segments at a null pointer", n_segs_total);
    NB_REQUIRE(((uintptr_t)segs & 15) == 0, "raster_batch: the segment rows must be 16-byte aligned");
    NB_REQUIRE(k >= 1 && h >= 1 && w >= 1, "raster_batch: bad sizes (%d x %d x %d)", k, h, w);
    NB_REQUIRE((long long)h * w < (1ll << 31), "raster_batch: image too large");
    const int ncx = nb_cdiv(w, NB_RASTER_CELL), ncy = nb_cdiv(h, NB_RASTER_CELL);
    const long long ncells = (long long)ncx * ncy;
    NB_REQUIRE(ncells * k < (1ll << 31), "raster_batch: %d drawings of %lld cells exceed the grid", k, ncells);
    hipLaunchKernelGGL(raster_batch_kernel, dim3((unsigned)(ncells * k)), dim3(256), 0, (hipStream_t)stream, segs, seg_off, n_segs_total,
                       out, h, w, off_y, off_x, ncx, (int)ncells);
    NB_CHECK_LAUNCH("raster_batch");
    return NB_OK;
}
