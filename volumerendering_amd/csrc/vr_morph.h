// vr_morph.h -- mask morphology and contour algebra on the device (vr_mask_morph, include/vr.h): one contour of a mask slot, restricted
// to a box, is dilated, eroded, closed or opened by a structuring element given as half-chords along x, or taken as it is, and the
// result is combined into a contour of a mask slot.  Exact set arithmetic: nothing can be fused, so vr_set_arithmetic plays no part and
// the kernels are compiled once, included by vr_api.hip alone.
//
// State: BIT-ROWS (vr_bitrows.h: their layout, the box walk, bit_pack_kernel which fills the operand A', the write's combine rule).
//
// Dilate (morph_dilate_kernel): one lane per output word, neighbouring lanes along x, then y.  The element's rows (dy, dz) come sorted
// by their half-chord h, largest first.  A three-word accumulator (the word and its two x neighbours) starts empty at level hmax; going
// down one level dilates it by one voxel along x, with carries between the three words, and at each level the source words of the rows
// whose half-chord equals that level are ORed in.  After level 0 the centre word is the output: a row with half-chord h has been
// x-dilated exactly h times, and since h <= 31 < 64 nothing beyond the two neighbour words can reach the centre.  A row with h == 0 is
// never shifted, so only its centre word is loaded.  Cost per output word: 3 loads per element row plus hmax shift-ORs.
// Erosion is the same kernel between complements (COMP): a source word is read as ~w & box and the result stored as ~acc & box, so
// that the outside of the box never erodes.  CLOSE and OPEN are two launches with ping-pong buffers; the launch boundary is the
// visibility point.  No kernel waits for another workgroup and nothing spins.
//
// Settling: a launch covers a REGION of the box only (words x rows x slices); the destination buffer is zeroed by a memset before it
// and keeps zeros outside the region.  The host picks a region outside of which the result is known to be empty (vr_api_morph.h): the
// bounding box of the source bits grown by the radii for a dilation, the bounding box itself for an erosion.
//
// Write (morph_write_kernel): one wavefront per word of the box, one lane per voxel, one 4-byte vector store into component
// dst_contour and only where `combine` stores something (BitCombine); words that store nothing are skipped.  |R| and its box
// from the R words.
#pragma once
#include "vr_bitrows.h"

namespace vr {

// The device words of one vr_mask_morph: set by the host before the first kernel, read behind the pack and the write.
struct MorphWords {
    CountBox src;     // |A'| and its bounding box (both start as CountBox::empty())
    CountBox result;  // |R| and its
};

// Kernel argument block of the dilation and the write of a vr_mask_morph (vr_morph_desc of include/vr.h): passed by value.
struct MorphParams {
    float4* dst;                  // the destination slot's x-fastest vec4 voxels
    int dst_contour;
    BitRows b;                    // the volume, the box and its words
    const unsigned long long* r;  // the result R (wx * ny * nz words, as every bit-row buffer)
    const unsigned* rows;         // the element's rows: h | (dy + 32) << 8 | (dz + 32) << 16, sorted by h, largest first
    int n_rows, hmax;
    BitCombine c;                 // how R is stored
    MorphWords* w;
};
// One dilation launch: from src into the words of a region of dst (rw words from word rw0, ry rows from ry0, rz slices from rz0).
struct MorphPass {
    const unsigned long long* src;
    unsigned long long* dst;
    int rw0, rw, ry0, ry, rz0, rz;
    unsigned long long words;     // rw * ry * rz
};

// the source word (xw, y, z) of a dilation; COMP: of the box's complement
template <bool COMP>
__device__ __forceinline__ unsigned long long morph_src_word(const MorphParams& P, const unsigned long long* src, int xw, int y, int z)
{
    if (xw < 0 || xw >= P.b.wx || y < P.b.lo[1] || y >= P.b.hi[1] || z < P.b.lo[2] || z >= P.b.hi[2]) return 0ull;
    const unsigned long long w = src[((size_t)z * (size_t)P.b.ny + (size_t)y) * (size_t)P.b.wx + (size_t)xw];
    if constexpr (COMP) return ~w & bit_xmask(xw, P.b.lo[0], P.b.hi[0]);
    return w;
}

template <bool COMP>
__global__ __launch_bounds__(256) void morph_dilate_kernel(const MorphParams P, const MorphPass S)
{
    const unsigned long long t = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
    if (t >= S.words) return;
    const unsigned long long row = t / (unsigned)S.rw;
    const int xw = S.rw0 + (int)(t - row * (unsigned)S.rw);
    const unsigned long long sl = row / (unsigned)S.ry;
    const int y = S.ry0 + (int)(row - sl * (unsigned)S.ry), z = S.rz0 + (int)sl;
    unsigned long long l = 0ull, c = 0ull, r = 0ull;
    int level = P.hmax;
    for (int i = 0; i < P.n_rows; ++i) {
        const unsigned e = P.rows[i];  // (uniform: h | (dy + 32) << 8 | (dz + 32) << 16, sorted by h, largest first)
        const int h = (int)(e & 0xFFu), dy = (int)((e >> 8) & 0xFFu) - 32, dz = (int)((e >> 16) & 0xFFu) - 32;
        for (; level > h; --level) {
            const unsigned long long nl = l | (l << 1) | (l >> 1) | (c << 63);
            const unsigned long long nr = r | (r << 1) | (r >> 1) | (c >> 63);
            c = c | (c << 1) | (c >> 1) | (l >> 63) | (r << 63);
            l = nl;
            r = nr;
        }
        c |= morph_src_word<COMP>(P, S.src, xw, y + dy, z + dz);
        if (h > 0) {
            l |= morph_src_word<COMP>(P, S.src, xw - 1, y + dy, z + dz);
            r |= morph_src_word<COMP>(P, S.src, xw + 1, y + dy, z + dz);
        }
    }
    for (; level > 0; --level) {
        const unsigned long long nl = l | (l << 1) | (l >> 1) | (c << 63);
        const unsigned long long nr = r | (r << 1) | (r >> 1) | (c >> 63);
        c = c | (c << 1) | (c >> 1) | (l >> 63) | (r << 63);
        l = nl;
        r = nr;
    }
    const unsigned long long box = bit_xmask(xw, P.b.lo[0], P.b.hi[0]);  // (the region's rows and slices are the box's)
    S.dst[((size_t)z * (size_t)P.b.ny + (size_t)y) * (size_t)P.b.wx + (size_t)xw] = (COMP ? ~c : c) & box;
}

__global__ __launch_bounds__(256) void morph_write_kernel(const MorphParams P)
{
    const unsigned lane = threadIdx.x & 63u;
    const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    float* const out = reinterpret_cast<float*>(P.dst) + P.dst_contour;
    CountBox n = CountBox::empty();  // (wave-uniform)
    const unsigned long long W = (unsigned long long)gridDim.x * 4ull;
    for (unsigned long long u = (unsigned long long)blockIdx.x * 4ull + wave; u < P.b.box_words; u += W) {
        int xw, y, z;
        bit_box_word(P.b, u, xw, y, z);
        const unsigned long long rw = P.r[((size_t)z * (size_t)P.b.ny + (size_t)y) * (size_t)P.b.wx + (size_t)xw];  // (zero outside the box)
        const unsigned long long st = P.c.stores(rw, bit_xmask(xw, P.b.lo[0], P.b.hi[0]));
        if (st != 0ull) {
            const bool set = (rw >> lane) & 1ull;
            if ((st >> lane) & 1ull) {
                const size_t idx = ((size_t)z * (size_t)P.b.ny + (size_t)y) * (size_t)P.b.nx + (size_t)(xw << 6) + (size_t)lane;
                out[idx * 4u] = P.c.value(set);
            }
        }
        bit_fold(rw, xw, y, z, n);
    }
    if (lane == 0u) report_count_box(&P.w->result, n.voxels, n.lo, n.hi);
}

}  // namespace vr
