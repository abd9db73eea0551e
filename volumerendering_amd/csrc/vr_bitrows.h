// vr_bitrows.h -- the BIT-ROW layer of the mask tools on the device (mask morphology vr_morph.h, distance maps vr_dist.h, polygon
// rasterisation vr_raster.h): what vr_units.h is to the brick tools.  One 64-bit word per 64 voxels along x, W[z][y][xw] with
// xw < wx = ceil(nx / 64), bit i of word xw = voxel x = 64 xw + i: 16 MiB for a 512^3 volume beside its 2 GiB of voxels.  Bits beyond nx
// or outside the box are zero in every buffer, always; the buffers are parts of ONE scratch of the context (vr_ctx::bit_row_scratch).
// Here: the box walk of the kernels that take one wavefront per word of the box and one lane per voxel (BitRows, bit_box_word), a word's
// box mask and its fold into a count and bounding box, the rule by which a write combines bits into a contour (BitCombine), and the
// pack of a contour (bit_pack_kernel): a word is ONE 64-bit ballot of in_box && v != 0.0f (vr_hist.h's membership rule: NaN is in,
// -0.0f is out), the count and the box of the packed bits come from the popcount and the first / last bit of the words.
#pragma once
#include "../../include/vr.h"
#include "vr_device.h"  // DevVolume
#include "vr_shared.h"  // vr_ballot
#include "vr_units.h"

namespace vr {

struct BitRows {  // (filled by bit_rows, vr_api_tools.h)
    int nx, ny, nz;                // of the volume
    int wx;                        // words per row: ceil(nx / 64)
    int lo[3], hi[3];              // the voxel box, half open (hi <= n)
    int bw0, bw;                   // the words of a row that meet the box: the first and their number ...
    unsigned long long box_words;  // ... and bw * rows * slices of the box (0 for an empty box)
    size_t words() const { return (size_t)wx * (size_t)ny * (size_t)nz; }  // of one buffer
};

// the bits of word xw whose voxels lie in [lo, hi) along x
__device__ __forceinline__ unsigned long long bit_xmask(int xw, int lo, int hi)
{
    const int a = max(lo - (xw << 6), 0), b = min(hi - (xw << 6), 64);  // bits [a, b)
    if (b <= a) return 0ull;
    const unsigned long long upto_b = b >= 64 ? ~0ull : ((1ull << b) - 1ull);
    return upto_b & ~((1ull << a) - 1ull);  // (a <= 63 here)
}

// folds one wavefront's word (its popcount, first and last bit, row and slice) into the words' count and bounding box; lane 0 alone
__device__ __forceinline__ void bit_fold(unsigned long long w, int xw, int y, int z, CountBox& n)
{
    if (w == 0ull) return;
    n.voxels += (unsigned long long)__popcll(w);
    n.lo[0] = min(n.lo[0], (xw << 6) + __ffsll((long long)w) - 1);
    n.hi[0] = max(n.hi[0], (xw << 6) + 64 - __clzll((long long)w));
    n.lo[1] = min(n.lo[1], y);
    n.hi[1] = max(n.hi[1], y + 1);
    n.lo[2] = min(n.lo[2], z);
    n.hi[2] = max(n.hi[2], z + 1);
}

// word u of the box's words -> (xw, y, z): B.bw words per row from word B.bw0, rows and slices of the box
__device__ __forceinline__ void bit_box_word(const BitRows& B, unsigned long long u, int& xw, int& y, int& z)
{
    const unsigned long long row = u / (unsigned)B.bw;
    xw = B.bw0 + (int)(u - row * (unsigned)B.bw);
    const unsigned rows = (unsigned)(B.hi[1] - B.lo[1]);
    const unsigned long long sl = row / rows;
    y = B.lo[1] + (int)(row - sl * rows);
    z = B.lo[2] + (int)sl;
}

// The COMBINE RULE of a write into a contour (include/vr.h states it for vr_mask_morph and vr_mask_polygons), for a word of the box
// whose result bits are rw (zero outside the box) and whose box mask is `box`.  Which voxels are stored: REPLACE all of the box (only R
// where the slot was created zeroed: `fresh`), OR and ANDNOT R, AND the rest; a word whose mask is zero is skipped.  What is stored,
// given the lane's bit of rw: 1.0f in R for REPLACE and OR, +0.0f wherever else something is stored.
struct BitCombine {
    int combine, fresh;  // VR_MORPH_REPLACE ..; the destination slot was created zeroed by this call
    __device__ __forceinline__ unsigned long long stores(unsigned long long rw, unsigned long long box) const
    {
        if (combine == VR_MORPH_REPLACE) return fresh ? rw : box;
        return combine == VR_MORPH_AND ? box & ~rw : rw;
    }
    __device__ __forceinline__ float value(bool set) const { return (set && combine <= VR_MORPH_OR) ? 1.0f : 0.0f; }
};

// Kernel argument block of a pack: passed by value.
struct BitPack {
    const float4* src;         // the source slot's x-fastest vec4 voxels ...
    int contour;               // ... and the component that is packed
    BitRows b;
    unsigned long long* bits;  // the packed bits (zeroed before)
    CountBox* n;               // their count and bounding box (starts as CountBox::empty())
};

__global__ __launch_bounds__(256) void bit_pack_kernel(const BitPack P)
{
    const unsigned lane = threadIdx.x & 63u;
    const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const float* const src = reinterpret_cast<const float*>(P.src) + P.contour;
    CountBox n = CountBox::empty();  // (wave-uniform)
    const unsigned long long W = (unsigned long long)gridDim.x * 4ull;
    for (unsigned long long u = (unsigned long long)blockIdx.x * 4ull + wave; u < P.b.box_words; u += W) {
        int xw, y, z;
        bit_box_word(P.b, u, xw, y, z);
        const int x = (xw << 6) + (int)lane;
        bool in = false;
        if (x >= P.b.lo[0] && x < P.b.hi[0]) {  // (hi <= n; y and z are the box's)
            const size_t idx = ((size_t)z * (size_t)P.b.ny + (size_t)y) * (size_t)P.b.nx + (size_t)x;
            in = src[idx * 4u] != 0.0f;
        }
        const unsigned long long w = vr_ballot(in);
        if (lane == 0u) P.bits[((size_t)z * (size_t)P.b.ny + (size_t)y) * (size_t)P.b.wx + (size_t)xw] = w;
        bit_fold(w, xw, y, z, n);
    }
    if (lane == 0u) report_count_box(P.n, n.voxels, n.lo, n.hi);
}

}  // namespace vr
