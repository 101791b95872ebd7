// Drawing preparation on the device for gfx950: everything between a decoded drawing and the padded, thresholded geometry the tiled
// schedule paints from, plus the crop + composite on white behind it.  Counterparts of the reference's host code:
//   _read_any_geo        forger/viz/paint_image_main.py:30-57   gray value, range stretch, Otsu threshold
//   threshold_img        forger/util/img_proc.py:66-71          (skimage.filters.threshold_otsu, one bin per integer value)
//   pad / tile picks     paint_image_main.py:58-61, forger/viz/style_transfer.py:15-48
//   --on_white           paint_image_main.py:179-183
// All of it is memory-bound byte processing.  One threshold step flips whole regions of the drawing, so every value is computed in
// the order and precision of the numpy code (painting.prepare_geometry_image): fp32 multiply, subtract and add as separate operations
// (the build has -ffp-contract=off), divisions formed in float64 and rounded once (53 >= 2 * 24 + 2 bits: the correctly rounded fp32
// quotient whatever the fp32 division options of the build), the Otsu statistics in float64 in numpy's summation order.
// The passes recompute the gray value from the drawing; there is no float image the size of the drawing.
#include "nb_common.h"
#include <cstdint>

namespace {

// scratch layout (NB_GEOM_PREP_WS_BYTES, include/neube_hip.h): uint32 words
constexpr int WS_MIN = 0, WS_MAX = 1, WS_THR = 2, WS_HIST = 4, WS_WORDS = WS_HIST + 256;
static_assert(WS_WORDS * 4 == NB_GEOM_PREP_WS_BYTES, "scratch layout and header constant disagree");

constexpr int PX = 4;            // consecutive pixels per thread and step: 4 / 12 / 16 bytes at 1 / 3 / 4 channels

// gray value of one pixel from its bytes (paint_image_main.py:38-46)
__device__ __forceinline__ float gray_of(int c0, int c1, int c2, int c3, int channels) {
    if (channels == 1) return (float)c0;
    const float mean = (float)((double)((c0 + c1) + c2) / 3.0);
    if (channels == 3) return mean;
    const float alpha = (float)((double)c3 / 255.0);
    const float a = mean * alpha;
    const float b = 255.f * (1.f - alpha);
    return a + b;
}

__device__ __forceinline__ float gray_at(const uint8_t* __restrict__ img, size_t pix, int channels) {
    const uint8_t* p = img + pix * channels;
    if (channels == 1) return gray_of(p[0], 0, 0, 0, 1);
    if (channels == 3) return gray_of(p[0], p[1], p[2], 0, 3);
    return gray_of(p[0], p[1], p[2], p[3], 4);
}

// gray values of the PX pixels from `pix` on (pix a multiple of PX, all inside the image): dword loads where the drawing is 4-byte aligned
__device__ __forceinline__ void gray_px(const uint8_t* __restrict__ img, size_t pix, int channels, bool aligned, float g[PX]) {
    if (!aligned) {
#pragma unroll
        for (int i = 0; i < PX; ++i) g[i] = gray_at(img, pix + i, channels);
        return;
    }
    const uint32_t* q = (const uint32_t*)(img + pix * channels);
    if (channels == 1) {
        const uint32_t v = q[0];
#pragma unroll
        for (int i = 0; i < PX; ++i) g[i] = (float)((v >> (8 * i)) & 255u);
    } else if (channels == 3) {
        const uint32_t a = q[0], b = q[1], c = q[2];          // r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3
        g[0] = gray_of(a & 255, (a >> 8) & 255, (a >> 16) & 255, 0, 3);
        g[1] = gray_of(a >> 24, b & 255, (b >> 8) & 255, 0, 3);
        g[2] = gray_of((b >> 16) & 255, b >> 24, c & 255, 0, 3);
        g[3] = gray_of((c >> 8) & 255, (c >> 16) & 255, c >> 24, 0, 3);
    } else {
#pragma unroll
        for (int i = 0; i < PX; ++i) {
            const uint32_t v = q[i];
            g[i] = gray_of(v & 255, (v >> 8) & 255, (v >> 16) & 255, v >> 24, 4);
        }
    }
}

// the range stretch of paint_image_main.py:48-55 for one value: subtract a positive minimum, scale a maximum below 255 up to 255,
// truncate.  `mn`, `mx` are the global extrema of the gray values; the maximum after the subtraction is mx - mn exactly (fp32
// subtraction of a constant is monotone), so one reduction pass serves both.
struct Stretch {
    float mn, scale;
    bool sub, mul;
    __device__ __forceinline__ Stretch(const uint32_t* __restrict__ ws) {
        mn = __uint_as_float(ws[WS_MIN]);
        float mx = __uint_as_float(ws[WS_MAX]);
        sub = mn > 0.f;
        if (sub) mx = mx - mn;
        mul = mx > 0.f && mx < 255.f;
        scale = mul ? (float)(255.0 / (double)mx) : 1.f;
    }
    __device__ __forceinline__ int operator()(float g) const {
        if (sub) g = g - mn;
        if (mul) g = g * scale;
        return (int)g & 255;
    }
};

__global__ __launch_bounds__(320) void prep_clear_kernel(uint32_t* __restrict__ ws) {
    const int i = threadIdx.x;
    if (i < WS_WORDS) ws[i] = (i == WS_MIN) ? 0x7f800000u : 0u;           // min starts at +inf; gray values are >= 0
}

// pass 1: global minimum and maximum of the gray values.  They are >= 0, so their bit patterns order like unsigned integers and
// integer atomics give the same answer in any order.
__global__ __launch_bounds__(256) void prep_minmax_kernel(const uint8_t* __restrict__ img, size_t npix, int channels, bool aligned,
                                                          uint32_t* __restrict__ ws) {
    uint32_t lo = 0x7f800000u, hi = 0u;
    const size_t nquad = npix / PX;
    for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < nquad; q += (size_t)gridDim.x * 256) {
        float g[PX];
        gray_px(img, q * PX, channels, aligned, g);
#pragma unroll
        for (int i = 0; i < PX; ++i) {
            const uint32_t b = __float_as_uint(g[i]);
            lo = b < lo ? b : lo;
            hi = b > hi ? b : hi;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < (int)(npix - nquad * PX)) {         // the last npix % PX pixels
        const uint32_t b = __float_as_uint(gray_at(img, nquad * PX + threadIdx.x, channels));
        lo = b < lo ? b : lo;
        hi = b > hi ? b : hi;
    }
    __shared__ uint32_t s_lo, s_hi;
    if (threadIdx.x == 0) { s_lo = 0x7f800000u; s_hi = 0u; }
    __syncthreads();
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t l2 = __shfl_xor(lo, o), h2 = __shfl_xor(hi, o);
        lo = l2 < lo ? l2 : lo;
        hi = h2 > hi ? h2 : hi;
    }
    if ((threadIdx.x & 63) == 0) { atomicMin(&s_lo, lo); atomicMax(&s_hi, hi); }
    __syncthreads();
    if (threadIdx.x == 0) { atomicMin(&ws[WS_MIN], s_lo); atomicMax(&ws[WS_MAX], s_hi); }
}

// pass 2: 256-bin histogram of the stretched uint8 image, integer counts (deterministic).  A drawing is almost entirely one value, so
// LDS atomics per pixel would serialise on that bin: every lane walks consecutive pixels and folds runs of equal values into one
// count, carried across its steps, and each wave adds into its own copy of the histogram.
__global__ __launch_bounds__(256) void prep_hist_kernel(const uint8_t* __restrict__ img, size_t npix, int channels, bool aligned,
                                                        uint32_t* __restrict__ ws) {
    __shared__ uint32_t s_hist[4][256];
    for (int i = threadIdx.x; i < 4 * 256; i += 256) (&s_hist[0][0])[i] = 0u;
    __syncthreads();
    const Stretch st(ws);
    uint32_t* mine = s_hist[threadIdx.x >> 6];
    int cur = -1;
    uint32_t run = 0;
    const size_t nquad = npix / PX;
    for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < nquad; q += (size_t)gridDim.x * 256) {
        float g[PX];
        gray_px(img, q * PX, channels, aligned, g);
#pragma unroll
        for (int i = 0; i < PX; ++i) {
            const int v = st(g[i]);
            if (v != cur) {
                if (run) atomicAdd(&mine[cur], run);
                cur = v;
                run = 0;
            }
            ++run;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < (int)(npix - nquad * PX)) {
        const int v = st(gray_at(img, nquad * PX + threadIdx.x, channels));
        if (v != cur) {
            if (run) atomicAdd(&mine[cur], run);
            cur = v;
            run = 0;
        }
        ++run;
    }
    if (run) atomicAdd(&mine[cur], run);
    __syncthreads();
    const uint32_t n = s_hist[0][threadIdx.x] + s_hist[1][threadIdx.x] + s_hist[2][threadIdx.x] + s_hist[3][threadIdx.x];
    if (n) atomicAdd(&ws[WS_HIST + threadIdx.x], n);
}

// pass 3: skimage's threshold_otsu over the occupied range lo..hi (painting.threshold_otsu): float64, cumulative sums in numpy's
// sequential order, var12 = (w1 * w2) * (m1 - m2)^2, first maximum.  One lane, about a thousand float64 operations.
__global__ __launch_bounds__(64) void prep_otsu_kernel(uint32_t* __restrict__ ws) {
    __shared__ double s_w2[257], s_s2[257];
    if (threadIdx.x != 0) return;
    const uint32_t* hist = ws + WS_HIST;
    int lo = 256, hi = -1;
    for (int v = 0; v < 256; ++v)
        if (hist[v]) {
            if (lo == 256) lo = v;
            hi = v;
        }
    if (hi < 0) { ws[WS_THR] = 0; return; }
    if (lo == hi) { ws[WS_THR] = (uint32_t)lo; return; }
    double w2 = 0.0, s2 = 0.0;
    for (int v = hi; v >= lo; --v) {                       // np.cumsum over the reversed arrays
        const double c = (double)hist[v];
        w2 = w2 + c;
        s2 = s2 + c * (double)v;
        s_w2[v] = w2;
        s_s2[v] = s2;
    }
    double w1 = 0.0, s1 = 0.0, best = 0.0;
    int arg = lo;
    for (int v = lo; v < hi; ++v) {
        const double c = (double)hist[v];
        w1 = w1 + c;
        s1 = s1 + c * (double)v;
        const double m1 = s1 / w1, m2 = s_s2[v + 1] / s_w2[v + 1];     // (both weights are >= one occupied end bin: never zero)
        const double d = m1 - m2;
        const double var = (w1 * s_w2[v + 1]) * (d * d);
        if (v == lo || var > best) { best = var; arg = v; }
    }
    ws[WS_THR] = (uint32_t)arg;
}

// pass 4: out = 255 outside the drawing's rectangle, inside it (stretched gray > threshold) ? 255 : 0.  PX consecutive bytes of `out`
// per thread, one dword store where `out` is 4-byte aligned.
__global__ __launch_bounds__(256) void prep_write_kernel(const uint8_t* __restrict__ img, int h, int w, int channels,
                                                         uint8_t* __restrict__ out, int out_w, size_t nout, int off_y, int off_x,
                                                         bool out_aligned, const uint32_t* __restrict__ ws) {
    const Stretch st(ws);
    const int thr = (int)ws[WS_THR];
    const size_t nquad = (nout + PX - 1) / PX;
    for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < nquad; q += (size_t)gridDim.x * 256) {
        const size_t o = q * PX;
        int y = (int)(o / (size_t)out_w) - off_y, x = (int)(o % (size_t)out_w) - off_x;
        uint32_t word = 0;
#pragma unroll
        for (int i = 0; i < PX; ++i) {
            uint32_t v = 255u;
            if (o + i < nout && y >= 0 && y < h && x >= 0 && x < w) v = st(gray_at(img, (size_t)y * w + x, channels)) > thr ? 255u : 0u;
            word |= v << (8 * i);
            if (++x == out_w - off_x) { x = -off_x; ++y; }
        }
        if (out_aligned && o + PX <= nout) {
            *(uint32_t*)(out + o) = word;
        } else {
#pragma unroll
            for (int i = 0; i < PX; ++i)
                if (o + i < nout) out[o + i] = (uint8_t)(word >> (8 * i));
        }
    }
}

int grid_for(size_t items) {                                   // 256 threads x PX items per step, at most 2048 workgroups
    const size_t g = (items + 256 * PX - 1) / (256 * PX);
    return g < 1 ? 1 : g > 2048 ? 2048 : (int)g;
}

}  // namespace

extern "C" int nb_geom_prepare_u8(const uint8_t* img, int h, int w, int channels, uint8_t* out, int out_h, int out_w, int off_y,
                                  int off_x, void* ws, void* stream) {
    NB_REQUIRE(img && out && ws, "geom_prepare: null pointer");
    NB_REQUIRE(channels == 1 || channels == 3 || channels == 4, "geom_prepare: %d channels (1, 3 or 4)", channels);
    NB_REQUIRE(h >= 1 && w >= 1 && out_h >= 1 && out_w >= 1, "geom_prepare: bad sizes (%d x %d into %d x %d)", h, w, out_h, out_w);
    NB_REQUIRE((long long)h * w < (1ll << 31) && (long long)out_h * out_w < (1ll << 31), "geom_prepare: image too large");
    NB_REQUIRE(off_y >= 0 && off_x >= 0 && (long long)off_y + h <= out_h && (long long)off_x + w <= out_w,
               "geom_prepare: %d x %d at (%d, %d) does not fit into %d x %d", h, w, off_y, off_x, out_h, out_w);
    NB_REQUIRE(((uintptr_t)ws & 3) == 0, "geom_prepare: scratch must be 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    uint32_t* wsw = (uint32_t*)ws;
    const size_t npix = (size_t)h * w, nout = (size_t)out_h * out_w;
    const bool aligned = ((uintptr_t)img & 3) == 0, out_aligned = ((uintptr_t)out & 3) == 0;
    hipLaunchKernelGGL(prep_clear_kernel, dim3(1), dim3(320), 0, s, wsw);
    NB_CHECK_LAUNCH("geom_prepare (clear)");
    hipLaunchKernelGGL(prep_minmax_kernel, dim3(grid_for(npix)), dim3(256), 0, s, img, npix, channels, aligned, wsw);
    NB_CHECK_LAUNCH("geom_prepare (min/max)");
    hipLaunchKernelGGL(prep_hist_kernel, dim3(grid_for(npix)), dim3(256), 0, s, img, npix, channels, aligned, wsw);
    NB_CHECK_LAUNCH("geom_prepare (histogram)");
    hipLaunchKernelGGL(prep_otsu_kernel, dim3(1), dim3(64), 0, s, wsw);
    NB_CHECK_LAUNCH("geom_prepare (otsu)");
    hipLaunchKernelGGL(prep_write_kernel, dim3(grid_for(nout)), dim3(256), 0, s, img, h, w, channels, out, out_w, nout, off_y, off_x,
                       out_aligned, (const uint32_t*)wsw);
    NB_CHECK_LAUNCH("geom_prepare (write)");
    return NB_OK;
}

// ------------------------------------------------------------------------------------------------
// stroke pixels per tile: the `np.sum(padded[y:y+P, x:x+P] < 0.001)` of style_transfer.py:40-44 for every tile of the grid in one
// launch, one workgroup per tile; pixels outside the image are background.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tile_stroke_counts_kernel(const uint8_t* __restrict__ geom, int gh, int gw, int r, int stride,
                                                                 int ncols, int32_t* __restrict__ counts) {
    const int tile = blockIdx.x;
    const int y0 = (tile / ncols) * stride, x0 = (tile % ncols) * stride;
    const int hh = min(r, gh - y0), ww = min(r, gw - x0);            // the part of the window inside the image
    int n = 0;
    if (hh > 0 && ww > 0)
        for (int i = threadIdx.x; i < hh * ww; i += 256) {
            const int y = i / ww, x = i - y * ww;
            n += geom[(size_t)(y0 + y) * gw + x0 + x] == 0;
        }
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o);
    __shared__ int s_n[4];
    if ((threadIdx.x & 63) == 0) s_n[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) counts[tile] = (s_n[0] + s_n[1]) + (s_n[2] + s_n[3]);
}

extern "C" int nb_tile_stroke_counts_u8(const uint8_t* geom, int gh, int gw, int r, int stride, int nrows, int ncols, int32_t* counts,
                                        void* stream) {
    NB_REQUIRE(geom && counts, "tile_stroke_counts: null pointer");
    NB_REQUIRE(gh >= 1 && gw >= 1 && r >= 1 && r <= 32768 && stride >= 1 && nrows >= 1 && ncols >= 1, "tile_stroke_counts: bad sizes");
    NB_REQUIRE((long long)nrows * ncols < (1ll << 24) && (long long)(nrows - 1) * stride < (1ll << 30) &&
               (long long)(ncols - 1) * stride < (1ll << 30), "tile_stroke_counts: grid too large");
    hipLaunchKernelGGL(tile_stroke_counts_kernel, dim3(nrows * ncols), dim3(256), 0, (hipStream_t)stream, geom, gh, gw, r, stride, ncols,
                       counts);
    NB_CHECK_LAUNCH("tile_stroke_counts");
    return NB_OK;
}

// ------------------------------------------------------------------------------------------------
// crop + composite on white (paint_image_main.py:179-183): out = trunc(clip(rgb * a + 255 * (1 - a), 0, 255)), a = alpha / 255
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void composite_on_white_kernel(const uint32_t* __restrict__ canvas, int cw, int y0, int x0, int h, int w,
                                                                 uint8_t* __restrict__ out) {
    const size_t n = (size_t)h * w;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const int y = (int)(i / (size_t)w), x = (int)(i - (size_t)y * w);
        const uint32_t v = canvas[(size_t)(y0 + y) * cw + x0 + x];
        const float a = (float)((double)(v >> 24) / 255.0);
        const float white = 255.f * (1.f - a);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float p = (float)((v >> (8 * c)) & 255u) * a;
            float f = p + white;
            f = f < 0.f ? 0.f : f > 255.f ? 255.f : f;
            out[i * 3 + c] = (uint8_t)(int)f;
        }
    }
}

extern "C" int nb_composite_on_white_u8(const uint8_t* canvas, int ch, int cw, int y0, int x0, int h, int w, uint8_t* out, void* stream) {
    NB_REQUIRE(canvas && out, "composite_on_white: null pointer");
    NB_REQUIRE(((uintptr_t)canvas & 3) == 0, "composite_on_white: the RGBA canvas must be 4-byte aligned");
    NB_REQUIRE(ch >= 1 && cw >= 1 && h >= 1 && w >= 1 && (long long)ch * cw < (1ll << 31), "composite_on_white: bad sizes");
    NB_REQUIRE(y0 >= 0 && x0 >= 0 && (long long)y0 + h <= ch && (long long)x0 + w <= cw,
               "composite_on_white: window %d x %d at (%d, %d) outside the %d x %d canvas", h, w, y0, x0, ch, cw);
    const size_t n = (size_t)h * w;
    const size_t g = (n + 255) / 256;
    hipLaunchKernelGGL(composite_on_white_kernel, dim3(g > 4096 ? 4096 : (int)g), dim3(256), 0, (hipStream_t)stream, (const uint32_t*)canvas,
                       cw, y0, x0, h, w, out);
    NB_CHECK_LAUNCH("composite_on_white");
    return NB_OK;
}

// ------------------------------------------------------------------------------------------------
// the tile grid of generate_stitching_crops (style_transfer.py:15-32) -- host only, no HIP call
// ------------------------------------------------------------------------------------------------
extern "C" int nb_stitching_grid(int h, int w, int patch_width, int overlap_margin, int* nrows, int* ncols, int* stride, int* padded_h,
                                 int* padded_w) {
    NB_REQUIRE(nrows && ncols && stride && padded_h && padded_w, "stitching_grid: null pointer");
    NB_REQUIRE(h >= 0 && w >= 0 && patch_width >= 1 && overlap_margin >= 0, "stitching_grid: bad sizes");
    const long long rw = (long long)patch_width - 2ll * overlap_margin;
    NB_REQUIRE(rw > 0, "stitching_grid: overlap margin %d too large for the patch width %d", overlap_margin, patch_width);
    const long long nr = h / rw + 1, nc = w / rw + 1;
    const long long ph = nr * rw + patch_width, pw = nc * rw + patch_width;
    NB_REQUIRE(ph < (1ll << 31) && pw < (1ll << 31), "stitching_grid: padded size overflows");
    *nrows = (int)nr; *ncols = (int)nc; *stride = (int)rw; *padded_h = (int)ph; *padded_w = (int)pw;
    return NB_OK;
}
