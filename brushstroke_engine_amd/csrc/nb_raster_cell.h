// One 64 x 64 cell of a capsule raster: the per-pixel arithmetic and the stores of nb_raster_segments_u8 (csrc/nb_strokes.hip) and
// nb_raster_batch_u8 (csrc/nb_drawings.hip).  Both kernels call nb_raster_cell with their own rows, output and cell, so the two
// entries give the same bytes on the same rows by construction.  Files that include this are compiled unfused and without SLP
// pairing (build.py FILE_FLAGS).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

constexpr int NB_RASTER_SEG_PITCH = 8;     // floats per segment row
constexpr int NB_RASTER_CELL = 64;         // a workgroup rasterises one CELL x CELL block of `out`
constexpr int NB_RASTER_CHUNK = 256;       // segments staged per step: one per thread

__device__ __forceinline__ bool nb_finite_f(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// Called by all 256 threads of a workgroup (it holds barriers) for the cell whose first pixel is (cy0, cx0) of out [out_h,out_w].
// The workgroup walks all segments in chunks of 256: every thread tests one segment's bounding box (grown by r) against the cell,
// the hits are compacted into an LDS list with one ballot per wave, and every thread then tests its 16 pixels -- 4 consecutive
// columns of rows ty, ty + 16, ty + 32, ty + 48, so that a wave's stores are whole 64-byte row pieces -- against the list.  The
// result is a union of per-pixel booleans: it does not depend on the order of the segments, and there are no atomics and no lists
// in global memory (cost: cells x segments box tests, 32 bytes each, served from L2).  Nothing outside segs[0 .. n_segs) rows and
// out[0 .. out_h * out_w) is addressed.
__device__ __forceinline__ void nb_raster_cell(const float* __restrict__ segs, unsigned n_segs, uint8_t* __restrict__ out, int out_h,
                                               int out_w, int off_y, int off_x, int cy0, int cx0, int clear) {
    constexpr int SEG_PITCH = NB_RASTER_SEG_PITCH, CELL = NB_RASTER_CELL, CHUNK = NB_RASTER_CHUNK;
    __shared__ float4 s_geo[CHUNK];        // x0, y0, ex, ey
    __shared__ float2 s_aux[CHUNK];        // 1 / |e|^2 (0 for a disc), r^2
    __shared__ int s_wave[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tx = (tid & 15) * 4, ty = tid >> 4;
    // the cell in drawing coordinates, grown by one pixel: the box test below rounds (far less than that) and must never lose a hit
    const int cy1 = min(cy0 + CELL, out_h) - 1, cx1 = min(cx0 + CELL, out_w) - 1;
    const float lo_x = (float)((long long)cx0 - off_x - 1), hi_x = (float)((long long)cx1 - off_x + 1);
    const float lo_y = (float)((long long)cy0 - off_y - 1), hi_y = (float)((long long)cy1 - off_y + 1);
    const float px0 = (float)((long long)cx0 + tx - off_x), py0 = (float)((long long)cy0 + ty - off_y);
    unsigned covered = 0;                  // bit 4 * k + i: pixel (row ty + 16 k, column tx + i)

    for (unsigned base = 0; base < n_segs; base += CHUNK) {
        const unsigned s = base + tid;
        bool hit = false;
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
        float r = 0.f;
        if (s < n_segs) {
            const float4* row = (const float4*)(segs + (size_t)s * SEG_PITCH);
            a = row[0];
            r = row[1].x;
            const bool ok = nb_finite_f(a.x) && nb_finite_f(a.y) && nb_finite_f(a.z) && nb_finite_f(a.w) && nb_finite_f(r) && r >= 0.f;
            hit = ok && fminf(a.x, a.z) - r <= hi_x && fmaxf(a.x, a.z) + r >= lo_x && fminf(a.y, a.w) - r <= hi_y &&
                  fmaxf(a.y, a.w) + r >= lo_y;
        }
        const unsigned long long m = __ballot(hit);
        if (lane == 0) s_wave[wave] = __popcll(m);
        __syncthreads();
        int pos = __popcll(m & ((1ull << lane) - 1ull)), total = 0;
        for (int w = 0; w < 4; ++w) {
            const int c = s_wave[w];
            if (w < wave) pos += c;
            total += c;
        }
        if (hit) {
            const float ex = a.z - a.x, ey = a.w - a.y;
            const float ee = ex * ex + ey * ey;
            s_geo[pos] = make_float4(a.x, a.y, ex, ey);
            s_aux[pos] = make_float2(ee > 0.f ? 1.f / ee : 0.f, r * r);
        }
        __syncthreads();
        if (covered != 0xffffu) {
            for (int i = 0; i < total; ++i) {
                const float4 g = s_geo[i];
                const float2 q = s_aux[i];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float dy = (py0 + (float)(16 * k)) - g.y;
                    const float dye = dy * g.w;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float dx = (px0 + (float)j) - g.x;       // (the pixel position is exact; one rounding)
                        float t = (dx * g.z + dye) * q.x;
                        t = fminf(fmaxf(t, 0.f), 1.f);                 // (a NaN from 0 * inf becomes 0)
                        const float fx = dx - t * g.z, fy = dy - t * g.w;
                        if (fx * fx + fy * fy <= q.y) covered |= 1u << (4 * k + j);
                    }
                }
            }
        }
        __syncthreads();                   // the list is rewritten by the next chunk
    }

    // stores: one dword per run of 4 where the run lies inside the row and its address is 4-byte aligned, bytes otherwise
    const int x = cx0 + tx;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int y = cy0 + ty + 16 * k;
        if (y >= out_h || x >= out_w) continue;
        const unsigned bits = (covered >> (4 * k)) & 15u;
        if (!clear && !bits) continue;
        uint8_t* p = out + (size_t)y * out_w + x;
        const bool whole = x + 4 <= out_w && ((uintptr_t)p & 3) == 0;
        if (clear) {
            uint32_t word = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) word |= ((bits >> j) & 1u ? 0u : 255u) << (8 * j);
            if (whole) {
                *(uint32_t*)p = word;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (x + j < out_w) p[j] = (uint8_t)(word >> (8 * j));
            }
        } else if (whole && bits == 15u) {
            *(uint32_t*)p = 0u;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (((bits >> j) & 1u) && x + j < out_w) p[j] = 0;
        }
    }
}
