// vr_raster.h -- polygon rasterisation on the device (vr_mask_polygons, include/vr.h): closed planar polygons, each on a slice of a grid,
// are scan-converted into the contours of a mask slot.  Exact integer arithmetic: nothing can be fused, so vr_set_arithmetic plays no
// part and the kernels are compiled once, included by vr_api.hip alone.
//
// State: BIT-ROWS (vr_bitrows.h: their layout, the box walk, the write's combine rule), one buffer R_k per contour, zeroed before the raster.
//
// Raster (raster_rows_kernel<UNION>): persistent workgroups of four wavefronts; a wavefront takes one work item at a time, a short run
// of rows of ONE polygon (the host derives the items from each polygon's y span cut to the box, vr_api_raster.h).  For a row j with
// centre ordinate yc the lanes stride over the polygon's edges, read from the uploaded points.  An edge that counts on the row
// (ay <= yc < by) toggles the voxels [0, k) of the row, k = ceil(N / D) with N = (yc - ay)(bx - ax) + (ax - ox)(by - ay) and
// D = sx (by - ay): one 64-bit division, then ONE bit, k - 1, flipped in a toggle row in LDS (LDS atomic XOR).  The row itself is the
// suffix XOR of the toggles: inside a word by shift-XORs, one lane per word; across the words of a chunk of 64 by the parity of the
// ballot of the word parities above the lane; across chunks, taken from the high end down, by a carried parity (rows wider than 4096
// voxels).  A row's crossings come in pairs, so nothing can be set outside the voxel span [s0, s1) of the polygon within the box: only
// the words of the span are in LDS, a toggle below s0 is dropped, one at or above s1 moves to s1 - 1, and the finished words are cut to
// the span.  They go into the contour's bit-rows with a 64-bit global atomic XOR (EVEN_ODD) or OR (UNION: the polygon's own even-odd
// row is complete in the wavefront before it is ORed, which is why an item never mixes polygons).  Both operations commute, so the
// bits do not depend on which wavefront takes which item.  No kernel waits for another workgroup and nothing spins; the launch boundary
// is the visibility point.
//
// Write (raster_write_kernel): one wavefront per word of the box, one lane per voxel; for each contour of `contours` one 4-byte vector
// store into its component and only where `combine` stores something (BitCombine, the rule of vr_mask_morph); words that store nothing are
// skipped.  |R_k| and the boxes from the R_k words.
#pragma once
#include "vr_bitrows.h"
#include "vr_shared.h"  // wave_lds_fence

namespace vr {

// One polygon of a vr_mask_polygons as the raster kernel reads it.
struct RasterPoly {
    unsigned first, count;  // its points: pts[first .. first + count)
    int slice, contour;
    int s0, s1;             // the voxels of a row it can set, within the box along x: [s0, s1), s0 < s1
};
// One work item of the raster kernel: `rows` rows from row j0 of polygon `poly`.
struct RasterItem {
    unsigned poly;
    unsigned short j0, rows;
};
// The device words of one vr_mask_polygons: |R_k| and its bounding box per contour (each starts as CountBox::empty()).
struct RasterWords {
    CountBox r[4];
};
// Kernel argument block of a vr_mask_polygons (vr_polygons_desc of include/vr.h): passed by value.
struct RasterParams {
    float4* dst;                   // the destination slot's x-fastest vec4 voxels
    BitRows b;                     // the volume, the box and its words
    BitCombine c;                  // how every R_k is stored
    unsigned long long* bits[4];   // the bit-rows R_k (wx * ny * nz words each, zeroed before the raster)
    int contours;                  // bit k: contour k is written
    long long ox, oy;              // the centre of voxel (0, 0)
    long long sx, sy;              // the voxel pitch
    const int2* pts;
    const RasterPoly* polys;
    const RasterItem* items;
    unsigned n_items;
    RasterWords* w;
};

constexpr int kRasterRowWords = 1024;  // the words of the longest row: 65535 voxels

template <bool UNION>
__global__ __launch_bounds__(256) void raster_rows_kernel(const RasterParams P)
{
    __shared__ unsigned long long s_toggles[4][kRasterRowWords];  // a wavefront's toggle row is its own: 32 KiB per workgroup
    const unsigned lane = threadIdx.x & 63u;
    const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    unsigned long long* const row = s_toggles[wave];
    const unsigned W = gridDim.x * 4u;
    for (unsigned it = blockIdx.x * 4u + wave; it < P.n_items; it += W) {
        const RasterItem I = P.items[it];  // (uniform)
        const RasterPoly G = P.polys[I.poly];
        const int w0 = G.s0 >> 6, nw = ((G.s1 - 1) >> 6) - w0 + 1;  // (0 <= s0 < s1 <= nx: 1 .. 1024 words)
        unsigned long long* const bits = G.contour == 0 ? P.bits[0] : G.contour == 1 ? P.bits[1] : G.contour == 2 ? P.bits[2] : P.bits[3];
        for (int j = (int)I.j0; j < (int)I.j0 + (int)I.rows; ++j) {
            const long long yc = P.oy + (long long)j * P.sy;
            for (int w = (int)lane; w < nw; w += 64) row[w] = 0ull;
            wave_lds_fence();
            for (unsigned e = lane; e < G.count; e += 64u) {
                int2 a = P.pts[G.first + e];
                int2 b = P.pts[G.first + (e + 1u == G.count ? 0u : e + 1u)];
                if (a.y > b.y) {
                    const int2 t = a;
                    a = b;
                    b = t;
                }
                if ((long long)a.y <= yc && yc < (long long)b.y) {  // (by > ay: a horizontal edge never passes)
                    const long long dy = (long long)b.y - (long long)a.y;
                    const long long N = (yc - (long long)a.y) * ((long long)b.x - (long long)a.x) + ((long long)a.x - P.ox) * dy;
                    if (N > 0) {  // (else k = 0: nothing is toggled)
                        const unsigned long long D = (unsigned long long)(P.sx * dy);
                        const unsigned long long k = ((unsigned long long)N + D - 1ull) / D;
                        if (k > (unsigned long long)G.s0) {  // bit k - 1 lies at or above s0
                            const int p = (int)(k < (unsigned long long)G.s1 ? k : (unsigned long long)G.s1) - 1;
                            atomicXor(&row[(p >> 6) - w0], 1ull << (p & 63));
                        }
                    }
                }
            }
            wave_lds_fence();
            unsigned carry = 0u;  // the parity of the toggles in the chunks above (uniform)
            for (int c = (nw - 1) >> 6; c >= 0; --c) {
                const int w = (c << 6) + (int)lane;
                unsigned long long s = w < nw ? row[w] : 0ull;
                s ^= s >> 1;
                s ^= s >> 2;
                s ^= s >> 4;
                s ^= s >> 8;
                s ^= s >> 16;
                s ^= s >> 32;  // bit x = the XOR of the word's toggles x .. 63; bit 0 = the word's parity
                const unsigned long long par = vr_ballot((s & 1ull) != 0ull);
                const unsigned long long above = lane == 63u ? 0ull : par >> (lane + 1u);
                if ((((unsigned)__popcll(above)) + carry) & 1u) s = ~s;
                carry ^= (unsigned)__popcll(par) & 1u;
                if (w < nw) {
                    s &= bit_xmask(w0 + w, G.s0, G.s1);
                    if (s != 0ull) {
                        unsigned long long* const dst = bits + ((size_t)G.slice * (size_t)P.b.ny + (size_t)j) * (size_t)P.b.wx + (size_t)(w0 + w);
                        if constexpr (UNION) atomicOr(dst, s);
                        else atomicXor(dst, s);
                    }
                }
            }
            wave_lds_fence();  // the row has been read before the next one zeroes it
        }
    }
}

__global__ __launch_bounds__(256) void raster_write_kernel(const RasterParams P)
{
    const unsigned lane = threadIdx.x & 63u;
    const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    float* const out = reinterpret_cast<float*>(P.dst);
    CountBox n[4] = {CountBox::empty(), CountBox::empty(), CountBox::empty(), CountBox::empty()};  // (wave-uniform)
    const unsigned long long W = (unsigned long long)gridDim.x * 4ull;
    for (unsigned long long u = (unsigned long long)blockIdx.x * 4ull + wave; u < P.b.box_words; u += W) {
        int xw, y, z;
        bit_box_word(P.b, u, xw, y, z);
        const size_t wi = ((size_t)z * (size_t)P.b.ny + (size_t)y) * (size_t)P.b.wx + (size_t)xw;
        const size_t idx = ((size_t)z * (size_t)P.b.ny + (size_t)y) * (size_t)P.b.nx + (size_t)(xw << 6) + (size_t)lane;
        const unsigned long long box = bit_xmask(xw, P.b.lo[0], P.b.hi[0]);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (!((P.contours >> k) & 1)) continue;
            const unsigned long long rw = P.bits[k][wi];  // (zero outside the box)
            const unsigned long long st = P.c.stores(rw, box);
            if (st != 0ull) {
                const bool set = (rw >> lane) & 1ull;
                if ((st >> lane) & 1ull) out[idx * 4u + (size_t)k] = P.c.value(set);
            }
            bit_fold(rw, xw, y, z, n[k]);
        }
    }
    if (lane == 0u) {
#pragma unroll
        for (int k = 0; k < 4; ++k) report_count_box(&P.w->r[k], n[k].voxels, n[k].lo, n[k].hi);
    }
}

}  // namespace vr
