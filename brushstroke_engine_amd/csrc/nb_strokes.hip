// Vector strokes on the device for gfx950: from stroke points to the thresholded geometry the tiled schedule paints from, with
// nothing the size of the canvas crossing PCIe.  Two entries:
//   nb_spline_flatten_f32    centripetal Catmull-Rom control points -> capsule segments (the curve of forger/core/curve.py:24-85,
//                            written from its mathematics: knots ts = cumsum(|dP|^alpha), the pyramid A1..A3 -> B1, B2 -> C)
//   nb_raster_segments_u8    capsule segments -> [out_h,out_w] uint8 geometry, 255 = background, 0 = stroke: what
//                            _read_any_geo + the padding of forger/viz/paint_image_main.py:30-61 produce from a drawn raster
// Coordinate convention: drawing coordinates are (x, y) in pixels; pixel (row y, column x) has its centre at exactly (x, y); pixel
// (Y, X) of the output buffer is the drawing position (X - off_x, Y - off_y).
// Segment rows: SEG_PITCH = 8 floats (32 bytes, two 16-byte loads): x0, y0, x1, y1, r, then three reserved floats that the
// rasteriser does not interpret (the flattener writes zeros).  A pixel is stroke iff its centre is within r of the closed segment
// for some row; a row with x0 == x1 and y0 == y1 is a disc; a row in which any of the five values is not finite, or r < 0, draws
// nothing.  Distances are formed relative to the segment's first point, differences first: pixel positions are exact integers in
// fp32, so the error of a distance is a few ulp of the distances involved (~1e-4 px at 8192) and not of the products.  Scalar fp32
// per pixel, unfused (-ffp-contract=off), no SLP pairing (build.py FILE_FLAGS).
#include "nb_common.h"
#include "nb_raster_cell.h"
#include <cstdint>

namespace {

constexpr int SEG_PITCH = NB_RASTER_SEG_PITCH;     // floats per segment row
constexpr int CELL = NB_RASTER_CELL;               // a workgroup rasterises one CELL x CELL block of `out`

// One 256-thread workgroup per 64 x 64 cell; the cell's work -- box tests, the LDS list, 16 pixels per thread, the stores -- is
// nb_raster_cell (nb_raster_cell.h), which nb_raster_batch_u8 (nb_drawings.hip) shares.
__global__ __launch_bounds__(256) void raster_segments_kernel(const float* __restrict__ segs, unsigned n_segs, uint8_t* __restrict__ out,
                                                              int out_h, int out_w, int off_y, int off_x, int ncx, int clear) {
    const int cy0 = ((int)blockIdx.x / ncx) * CELL, cx0 = ((int)blockIdx.x % ncx) * CELL;
    nb_raster_cell(segs, n_segs, out, out_h, out_w, off_y, off_x, cy0, cx0, clear);
}

// One thread per sample point of the flattened curves.  Stroke s with P_s control points has P_s - 3 spans of `subdiv` pieces and
// (P_s - 3) * subdiv + 1 sample points; its first segment row is (stroke_off[s] - 3 s) * subdiv and its first sample
// (stroke_off[s] - 3 s) * subdiv + s, both closed forms of the offsets: the thread finds its stroke by bisection, no scan, no atomics.
// Sample k of a stroke is evaluated ONCE and written as the start of segment k and the end of segment k - 1 (bit-equal: watertight
// polylines).  The knots of a span are local -- t0 = 0, then the three |dP|^alpha added up -- which is the reference's cumulative
// sum shifted by a constant the pyramid does not see.  A repeated control point makes a knot interval zero and the samples of the
// (up to three) spans that divide by it non-finite; the rasteriser draws nothing for such rows.
// Every index read from stroke_off is checked against the totals the host passed before it addresses anything.
__global__ __launch_bounds__(256) void spline_flatten_kernel(const float* __restrict__ ctrl, const int32_t* __restrict__ stroke_off,
                                                             int n_points, int n_strokes, int subdiv, float alpha,
                                                             float* __restrict__ segs, long long n_rows, long long n_samples) {
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= n_samples) return;
    auto first_sample = [&](int s) -> long long { return ((long long)stroke_off[s] - 3ll * s) * subdiv + s; };
    int lo = 0, hi = n_strokes;                                 // the last stroke whose first sample is <= g
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (first_sample(mid) <= g) lo = mid; else hi = mid;
    }
    const int s = lo;
    const long long p_begin = stroke_off[s], p_end = stroke_off[s + 1];
    if (p_begin < 0 || p_end > n_points || p_end - p_begin < 4) return;          // a malformed table writes nothing
    const long long nspans = p_end - p_begin - 3, nseg = nspans * subdiv;
    const long long k = g - first_sample(s);
    if (k < 0 || k > nseg) return;
    const long long row0 = (p_begin - 3ll * s) * subdiv;
    if (row0 < 0 || row0 + nseg > n_rows) return;
    long long span = k / subdiv;
    if (span >= nspans) span = nspans - 1;                      // the stroke's last sample: the end of its last span
    const int j = (int)(k - span * subdiv);

    const float* c = ctrl + (size_t)(p_begin + span) * 3;
    const float x0 = c[0], y0 = c[1], x1 = c[3], y1 = c[4], r1 = c[5], x2 = c[6], y2 = c[7], r2 = c[8], x3 = c[9], y3 = c[10];
    auto knot = [&](float ax, float ay, float bx, float by) -> float {
        const float dx = bx - ax, dy = by - ay;
        return powf(sqrtf(dx * dx + dy * dy), alpha);
    };
    const float t0 = 0.f, t1 = knot(x0, y0, x1, y1), t2 = t1 + knot(x1, y1, x2, y2), t3 = t2 + knot(x2, y2, x3, y3);
    const float u = (float)j / (float)subdiv;
    const float t = j == subdiv ? t2 : t1 + (t2 - t1) * u;
    // the pyramid: every level interpolates its two inputs linearly over the knot interval they span
    auto lerp = [&](float ta, float tb, float pa, float pb) -> float { return (tb - t) / (tb - ta) * pa + (t - ta) / (tb - ta) * pb; };
    const float a1x = lerp(t0, t1, x0, x1), a1y = lerp(t0, t1, y0, y1);
    const float a2x = lerp(t1, t2, x1, x2), a2y = lerp(t1, t2, y1, y2);
    const float a3x = lerp(t2, t3, x2, x3), a3y = lerp(t2, t3, y2, y3);
    const float b1x = lerp(t0, t2, a1x, a2x), b1y = lerp(t0, t2, a1y, a2y);
    const float b2x = lerp(t1, t3, a2x, a3x), b2y = lerp(t1, t3, a2y, a3y);
    const float cx = lerp(t1, t2, b1x, b2x), cy = lerp(t1, t2, b1y, b2y);

    if (k < nseg) {                                             // start of segment k; its radius at the piece's mid t
        float4* row = (float4*)(segs + (size_t)(row0 + k) * SEG_PITCH);
        float2* xy = (float2*)row;
        xy[0] = make_float2(cx, cy);
        const float um = ((float)j + 0.5f) / (float)subdiv;
        row[1] = make_float4(r1 + (r2 - r1) * um, 0.f, 0.f, 0.f);
    }
    if (k > 0) {                                                // end of segment k - 1
        float2* xy = (float2*)(segs + (size_t)(row0 + k - 1) * SEG_PITCH);
        xy[1] = make_float2(cx, cy);
    }
}

long long segment_count(long long n_points_total, long long n_strokes, long long subdiv) {
    return (n_points_total - 3 * n_strokes) * subdiv;
}

}  // namespace

extern "C" int nb_raster_segments_u8(const float* segs, int n_segs, uint8_t* out, int out_h, int out_w, int off_y, int off_x, int clear,
                                     void* stream) {
    NB_REQUIRE(out, "raster_segments: null pointer");
    NB_REQUIRE(n_segs >= 0 && (segs || n_segs == 0), "raster_segments: %d segments at a null pointer", n_segs);
    NB_REQUIRE(((uintptr_t)segs & 15) == 0, "raster_segments: the segment rows must be 16-byte aligned");
    NB_REQUIRE(out_h >= 1 && out_w >= 1, "raster_segments: bad sizes (%d x %d)", out_h, out_w);
    NB_REQUIRE((long long)out_h * out_w < (1ll << 31), "raster_segments: image too large");
    NB_REQUIRE(clear == 0 || clear == 1, "raster_segments: clear must be 0 or 1, got %d", clear);
    if (!clear && n_segs == 0) return NB_OK;                    // nothing to draw, nothing to fill
    const int ncx = nb_cdiv(out_w, CELL), ncy = nb_cdiv(out_h, CELL);
    hipLaunchKernelGGL(raster_segments_kernel, dim3((unsigned)ncx * (unsigned)ncy), dim3(256), 0, (hipStream_t)stream, segs,
                       (unsigned)n_segs, out, out_h, out_w, off_y, off_x, ncx, clear);
    NB_CHECK_LAUNCH("raster_segments");
    return NB_OK;
}

extern "C" long long nb_spline_segment_count(int n_points_total, int n_strokes, int subdiv) {
    NB_REQUIRE(n_strokes >= 0 && subdiv >= 1 && (long long)n_points_total >= 4ll * n_strokes,
               "spline_segment_count: %d points in %d strokes (at least 4 each), subdiv %d", n_points_total, n_strokes, subdiv);
    return segment_count(n_points_total, n_strokes, subdiv);
}

extern "C" int nb_spline_flatten_f32(const float* ctrl, const int32_t* stroke_off, int n_points_total, int n_strokes, int subdiv,
                                     float alpha, float* segs, int seg_capacity, void* stream) {
    NB_REQUIRE(ctrl && stroke_off && segs, "spline_flatten: null pointer");
    NB_REQUIRE(((uintptr_t)segs & 15) == 0, "spline_flatten: the segment rows must be 16-byte aligned");
    NB_REQUIRE(n_strokes >= 1 && subdiv >= 1 && (long long)n_points_total >= 4ll * n_strokes,
               "spline_flatten: %d points in %d strokes (at least 4 each), subdiv %d", n_points_total, n_strokes, subdiv);
    NB_REQUIRE(alpha >= 0.f && alpha <= 1.f, "spline_flatten: alpha %g outside [0, 1]", (double)alpha);
    const long long n_rows = segment_count(n_points_total, n_strokes, subdiv);
    NB_REQUIRE(n_rows < (1ll << 31) - (long long)n_strokes, "spline_flatten: too many segments");
    NB_REQUIRE((long long)seg_capacity >= n_rows, "spline_flatten: %lld segments do not fit into a capacity of %d", n_rows, seg_capacity);
    const long long n_samples = n_rows + n_strokes;
    hipLaunchKernelGGL(spline_flatten_kernel, dim3((unsigned)((n_samples + 255) / 256)), dim3(256), 0, (hipStream_t)stream, ctrl,
                       stroke_off, n_points_total, n_strokes, subdiv, alpha, segs, n_rows, n_samples);
    NB_CHECK_LAUNCH("spline_flatten");
    return NB_OK;
}
