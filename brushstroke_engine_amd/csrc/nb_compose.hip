// Compositing kernels of the paint session for gfx950 (painting.PaintSession): source-over / destination-out of rendered RGBA8 tiles
// onto a canvas that stays on the device, and a reduced view of a canvas window for previews.  Counterpart of what the reference
// leaves to its browser client: putImageData of the returned patches into a foreground layer (forger/ui/js/main_controller.js:776),
// drawn over the background canvas when the stroke ends (main_controller.js:131-141).
//
// Both kernels are exact integer arithmetic on straight-alpha RGBA8 (the contracts are in include/neube_hip.h; painting.py restates
// them in numpy, byte for byte), pointwise and bound by HBM.  The canvas is read and written in 16-byte vectors -- four pixels per
// lane, consecutive lanes on consecutive addresses, a wave on 1 KiB of one canvas row -- whenever it is 16-byte aligned with a width
// that is a multiple of four pixels (the session's canvases are); any other canvas takes the same kernels at one pixel per lane.
//
// nb_canvas_view_u8 is the PREVIEW path (a 4096^2 canvas reduced to 512^2 before it crosses PCIe): alpha-weighted integer means with
// round-half-up.  The exported image keeps nb_composite_on_white_u8 (nb_geomprep.hip) and the reference's float rounding.
#include "nb_common.h"
#include <cstdint>

// floor(num / den) for 0 < den, num < 2^25 and a quotient below 2^10: the fp32 estimate num * rcp(den) is within 2^-11 of the exact
// quotient (the conversion of num, the reciprocal and the product are each good to ~2^-22 relative), so its floor is off by at most
// one either way; the signed remainder says which.  Integer division proper is ~40 instructions on this hardware, and the over kernel
// divides three times per pixel.
__device__ __forceinline__ uint32_t nb_div_small(uint32_t num, uint32_t den, float rcp_den) {
    int q = (int)((float)num * rcp_den);
    int rem = (int)num - q * (int)den;
    if (rem < 0) { --q; rem += (int)den; }
    if (rem >= (int)den) ++q;
    return (uint32_t)q;
}

__device__ __forceinline__ uint32_t nb_div255(uint32_t v) { return v / 255u; }       // (a constant divisor: multiply and shift)

// one pixel of the contract of nb_over_tiles_u8: s over / out of d
__device__ __forceinline__ uint32_t nb_over_pixel(uint32_t s, uint32_t d, int mode, uint32_t opacity) {
    const uint32_t ae = nb_div255((s >> 24) * opacity + 127u), ad = d >> 24;
    const uint32_t t = ad * (255u - ae);
    if (mode == 1) return (d & 0x00ffffffu) | (nb_div255(t + 127u) << 24);
    // the three cases most pixels of a stroke are, and what the formula below gives for them: nothing to put over (the destination stays,
    // without a colour where it is transparent), nothing underneath (cs, ae), an opaque source
    if (ae == 0u) return ad ? d : 0u;
    if (ad == 0u || ae == 255u) return (s & 0x00ffffffu) | (ae << 24);
    const uint32_t den = ae * 255u + t;
    const float rcp = __builtin_amdgcn_rcpf((float)den);
    const uint32_t ws = ae * 255u, half = den >> 1;
    uint32_t out = nb_div255(den + 127u) << 24;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const uint32_t cs = (s >> (8 * c)) & 255u, cd = (d >> (8 * c)) & 255u;
        out |= nb_div_small(cs * ws + cd * t + half, den, rcp) << (8 * c);
    }
    return out;
}

// ------------------------------------------------------------------------------------------------
// tiles over the canvas.  A workgroup is one cell row (NB_CELL_H = 4 canvas rows, one wave each) of PX horizontally adjacent cells;
// a lane owns PX consecutive pixels, which lie in one cell.  Per pixel the cell's tiles are walked from the last to the first, as
// paste_tiles_kernel (nb_canvas.hip) does; the first interior that covers the pixel is its source.
// ------------------------------------------------------------------------------------------------
struct OverParams {
    const uint32_t* tiles;
    const int* dst_yx;
    uint32_t* canvas;
    const int* cell_off;
    const int* cell_tiles;
    int t, r, crop, h, w, cells_per_row, cell_x0, cell_y0, cells_x, mode, opacity;
};

template <int PX>
__global__ __launch_bounds__(256) void over_tiles_kernel(OverParams p) {
    static_assert(PX == 1 || PX == 4, "one pixel or one 16-byte vector per lane");
    const int lane = threadIdx.x & 63;
    const int rel_cell = blockIdx.x * PX + (lane * PX) / NB_CELL_W;        // cell column inside the box
    if (rel_cell >= p.cells_x) return;
    const int cell_col = p.cell_x0 + rel_cell, cell_row = p.cell_y0 + blockIdx.y;
    const int cx = cell_col * NB_CELL_W + (lane * PX) % NB_CELL_W;
    const int cy = cell_row * NB_CELL_H + (threadIdx.x >> 6);
    if (cx >= p.w || cy >= p.h) return;                                   // (PX = 4: w % 4 == 0, so the whole vector is inside)
    const int cell = cell_row * p.cells_per_row + cell_col;
    const int k0 = p.cell_off[cell], k1 = p.cell_off[cell + 1];
    uint32_t src[PX];
    unsigned found = 0;
    for (int k = k1 - 1; k >= k0 && found != (1u << PX) - 1u; --k) {
        const int t = p.cell_tiles[k];
        if ((unsigned)t >= (unsigned)p.t) continue;
        const int ly = cy - p.dst_yx[2 * t], lx = cx - p.dst_yx[2 * t + 1];
        if (ly < p.crop || ly >= p.r - p.crop) continue;
        const uint32_t* row = p.tiles + ((size_t)t * p.r + ly) * p.r;
#pragma unroll
        for (int i = 0; i < PX; ++i)
            if (!(found >> i & 1u) && lx + i >= p.crop && lx + i < p.r - p.crop) {
                src[i] = row[lx + i];
                found |= 1u << i;
            }
    }
    if (!found) return;
    const size_t pix = (size_t)cy * p.w + cx;
    if constexpr (PX == 4) {
        uint4 d = *reinterpret_cast<const uint4*>(p.canvas + pix);
        if (found & 1u) d.x = nb_over_pixel(src[0], d.x, p.mode, p.opacity);
        if (found & 2u) d.y = nb_over_pixel(src[1 % PX], d.y, p.mode, p.opacity);
        if (found & 4u) d.z = nb_over_pixel(src[2 % PX], d.z, p.mode, p.opacity);
        if (found & 8u) d.w = nb_over_pixel(src[3 % PX], d.w, p.mode, p.opacity);
        *reinterpret_cast<uint4*>(p.canvas + pix) = d;
    } else {
        p.canvas[pix] = nb_over_pixel(src[0], p.canvas[pix], p.mode, p.opacity);
    }
}

extern "C" int nb_over_tiles_u8(const uint8_t* tiles, int t, int r, const int32_t* dst_yx, int crop, uint8_t* canvas, int h, int w,
                                const int32_t* cell_off, const int32_t* cell_tiles, int cell_x0, int cell_y0, int cells_x, int cells_y,
                                int mode, int opacity, void* stream) {
    NB_REQUIRE(tiles && dst_yx && canvas && cell_off && cell_tiles, "over_tiles: null pointer");
    NB_REQUIRE((((uintptr_t)tiles | (uintptr_t)canvas) & 3) == 0, "over_tiles: RGBA tiles and canvas must be 4-byte aligned");
    NB_REQUIRE(t >= 1 && r >= 1 && h >= 1 && w >= 1 && crop >= 0 && 2 * crop < r, "over_tiles: bad sizes");
    NB_REQUIRE((long long)h * w < (1ll << 31) && (long long)t * r * r < (1ll << 40), "over_tiles: canvas or tiles too large");
    NB_REQUIRE(mode == 0 || mode == 1, "over_tiles: mode %d is neither 0 (paint) nor 1 (erase)", mode);
    NB_REQUIRE(opacity >= 0 && opacity <= 255, "over_tiles: opacity %d outside 0..255", opacity);
    const int cpr = nb_cdiv(w, NB_CELL_W), cpc = nb_cdiv(h, NB_CELL_H);
    NB_REQUIRE(cell_x0 >= 0 && cell_y0 >= 0 && cells_x >= 1 && cells_y >= 1 && (long long)cell_x0 + cells_x <= cpr &&
               (long long)cell_y0 + cells_y <= cpc, "over_tiles: cell box outside the canvas");
    NB_REQUIRE(cells_y <= 65535, "over_tiles: canvas too large");
    OverParams p{(const uint32_t*)tiles, dst_yx, (uint32_t*)canvas, cell_off, cell_tiles, t, r, crop, h, w, cpr, cell_x0, cell_y0, cells_x,
                 mode, opacity};
    if (((uintptr_t)canvas & 15) == 0 && w % 4 == 0)
        hipLaunchKernelGGL(over_tiles_kernel<4>, dim3(nb_cdiv(cells_x, 4), cells_y), dim3(256), 0, (hipStream_t)stream, p);
    else
        hipLaunchKernelGGL(over_tiles_kernel<1>, dim3(cells_x, cells_y), dim3(256), 0, (hipStream_t)stream, p);
    NB_CHECK_LAUNCH("over_tiles");
    return NB_OK;
}

// ------------------------------------------------------------------------------------------------
// reduced view of a canvas window.  A workgroup produces a few output rows of one strip of output columns.  Per output row its
// lanes read the k input rows of the strip in coalesced vectors (a lane keeps the column sums SA = sum a and SC = sum c * a of its PX
// columns in registers), hand the column sums over through the LDS, and the k columns of an output pixel are added up from there: no
// lane walks a k x k block of scattered bytes, and the strip may start at any pixel of the canvas.  At k = 1 there is nothing to add
// up: a lane turns its own pixels into output pixels, without the LDS and its barriers.
// ------------------------------------------------------------------------------------------------
#define NB_VIEW_COLS 1024        // input columns of a strip: 256 lanes x 4 pixels (at one pixel per lane a quarter of it is used)

struct ViewParams {
    const uint32_t* canvas;
    uint8_t* out;
    int cw, y0, x0, h, w, k, on_white, oh, ow, strip_out, rows_per_block;
};

// one output pixel of the contract of nb_canvas_view_u8 from the sums of its block of n pixels
__device__ __forceinline__ void nb_view_store(const ViewParams& p, size_t opix, uint32_t sc0, uint32_t sc1, uint32_t sc2, uint32_t sa,
                                              uint32_t n) {
    if (p.on_white) {
        const uint32_t den = 255u * n, white = 255u * (den - sa) + den / 2u;
        const float rcp = __builtin_amdgcn_rcpf((float)den);
        uint8_t* dst = p.out + opix * 3;
        dst[0] = (uint8_t)nb_div_small(sc0 + white, den, rcp);
        dst[1] = (uint8_t)nb_div_small(sc1 + white, den, rcp);
        dst[2] = (uint8_t)nb_div_small(sc2 + white, den, rcp);
    } else {
        uint32_t px = nb_div_small(sa + n / 2u, n, __builtin_amdgcn_rcpf((float)n)) << 24;
        if (sa > 0u) {
            const float rcp = __builtin_amdgcn_rcpf((float)sa);
            px |= nb_div_small(sc0 + sa / 2u, sa, rcp) | nb_div_small(sc1 + sa / 2u, sa, rcp) << 8 |
                  nb_div_small(sc2 + sa / 2u, sa, rcp) << 16;
        }
        reinterpret_cast<uint32_t*>(p.out)[opix] = px;
    }
}

template <int PX>
__device__ __forceinline__ void nb_view_load(const uint32_t* src, uint32_t (&v)[PX]) {
    if constexpr (PX == 4) {
        const uint4 q = *reinterpret_cast<const uint4*>(src);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
        v[0] = *src;
    }
}

template <int PX>
__global__ __launch_bounds__(256) void canvas_view_kernel(ViewParams p) {
    __shared__ uint4 sums[NB_VIEW_COLS];                                   // per input column of the strip: SC r, g, b and SA
    const int k = p.k;
    const int ox0 = blockIdx.x * p.strip_out;                             // first output column of the strip
    const int n_out = min(p.strip_out, p.ow - ox0);
    const int xs = p.x0 + ox0 * k;                                        // first input column (canvas coordinates) ...
    const int n_in = min(n_out * k, p.x0 + p.w - xs);                     // ... and how many the strip has inside the window
    const int xa = PX == 4 ? (xs & ~3) : xs;                              // where the aligned vectors start
    const int lx = xa + (int)threadIdx.x * PX;                            // this lane's first column
    const bool loads = lx < xs + n_in && lx + PX > xs;
    const int oy_end = min(p.oh, ((int)blockIdx.y + 1) * p.rows_per_block);
    if (k == 1) {
        if (!loads) return;
        for (int oy = blockIdx.y * p.rows_per_block; oy < oy_end; ++oy) {
            uint32_t v[PX];
            nb_view_load<PX>(p.canvas + (size_t)(p.y0 + oy) * p.cw + lx, v);
#pragma unroll
            for (int i = 0; i < PX; ++i) {
                const int col = lx + i - xs;
                const uint32_t a = v[i] >> 24;
                if (col >= 0 && col < n_in)
                    nb_view_store(p, (size_t)oy * p.ow + ox0 + col, (v[i] & 255u) * a, ((v[i] >> 8) & 255u) * a, ((v[i] >> 16) & 255u) * a, a, 1u);
            }
        }
        return;
    }
    for (int oy = blockIdx.y * p.rows_per_block; oy < oy_end; ++oy) {
        const int rows = min(k, p.h - oy * k);
        if (loads) {
            uint32_t acc[PX][4];
#pragma unroll
            for (int i = 0; i < PX; ++i) acc[i][0] = acc[i][1] = acc[i][2] = acc[i][3] = 0u;
            const uint32_t* src = p.canvas + (size_t)(p.y0 + oy * k) * p.cw + lx;
            for (int j = 0; j < rows; ++j, src += p.cw) {
                uint32_t v[PX];
                nb_view_load<PX>(src, v);
#pragma unroll
                for (int i = 0; i < PX; ++i) {
                    const uint32_t a = v[i] >> 24;
                    acc[i][0] += (v[i] & 255u) * a;
                    acc[i][1] += ((v[i] >> 8) & 255u) * a;
                    acc[i][2] += ((v[i] >> 16) & 255u) * a;
                    acc[i][3] += a;
                }
            }
#pragma unroll
            for (int i = 0; i < PX; ++i) {
                const int col = lx + i - xs;
                if (col >= 0 && col < n_in) sums[col] = make_uint4(acc[i][0], acc[i][1], acc[i][2], acc[i][3]);
            }
        }
        __syncthreads();
        for (int o = threadIdx.x; o < n_out; o += 256) {
            const int c0 = o * k, cols = min(k, n_in - c0);
            uint32_t sc0 = 0u, sc1 = 0u, sc2 = 0u, sa = 0u;
            for (int c = 0; c < cols; ++c) {
                const uint4 s = sums[c0 + c];
                sc0 += s.x; sc1 += s.y; sc2 += s.z; sa += s.w;
            }
            const uint32_t n = (uint32_t)(rows * cols);
            const size_t opix = (size_t)oy * p.ow + ox0 + o;
            nb_view_store(p, opix, sc0, sc1, sc2, sa, n);
        }
        __syncthreads();
    }
}

extern "C" int nb_canvas_view_u8(const uint8_t* canvas, int ch, int cw, int y0, int x0, int h, int w, int k, int on_white, uint8_t* out,
                                 void* stream) {
    NB_REQUIRE(canvas && out, "canvas_view: null pointer");
    NB_REQUIRE(((uintptr_t)canvas & 3) == 0, "canvas_view: the RGBA canvas must be 4-byte aligned");
    NB_REQUIRE(on_white == 0 || on_white == 1, "canvas_view: on_white must be 0 or 1");
    NB_REQUIRE(on_white == 1 || ((uintptr_t)out & 3) == 0, "canvas_view: the RGBA view must be 4-byte aligned");
    NB_REQUIRE(ch >= 1 && cw >= 1 && h >= 1 && w >= 1 && (long long)ch * cw < (1ll << 31), "canvas_view: bad sizes");
    NB_REQUIRE(k >= 1 && k <= 16, "canvas_view: factor %d outside 1..16", k);
    NB_REQUIRE(y0 >= 0 && x0 >= 0 && (long long)y0 + h <= ch && (long long)x0 + w <= cw,
               "canvas_view: window %d x %d at (%d, %d) outside the %d x %d canvas", h, w, y0, x0, ch, cw);
    const int oh = nb_cdiv(h, k), ow = nb_cdiv(w, k);
    const bool vec = ((uintptr_t)canvas & 15) == 0 && cw % 4 == 0;
    // output columns per strip: their k input columns each, plus up to three pixels in front of an aligned vector, fit the lanes
    const int strip_out = vec ? (NB_VIEW_COLS - 3) / k : 256 / k;
    const int rows_per_block = k == 1 ? 4 : k >= 16 ? 1 : 16 / k;         // ~16 input rows per workgroup; 4 where no barrier separates them
    ViewParams p{(const uint32_t*)canvas, out, cw, y0, x0, h, w, k, on_white, oh, ow, strip_out, rows_per_block};
    const dim3 grid(nb_cdiv(ow, strip_out), nb_cdiv(oh, rows_per_block));
    NB_REQUIRE(grid.y <= 65535, "canvas_view: window too large");
    if (vec)
        hipLaunchKernelGGL(canvas_view_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, p);
    else
        hipLaunchKernelGGL(canvas_view_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, p);
    NB_CHECK_LAUNCH("canvas_view");
    return NB_OK;
}
