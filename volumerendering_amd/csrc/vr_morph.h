// vr_morph.h -- mask morphology and contour algebra on the device (vr_mask_morph, include/vr.h): one contour of a mask slot, restricted
// to a box, is dilated, eroded, closed or opened by a structuring element given as half-chords along x, or taken as it is, and the
// result is combined into a contour of a mask slot.  Exact set arithmetic: nothing can be fused, so vr_set_arithmetic plays no part and
// the kernels are compiled once, included by vr_api.hip alone.
//
// State: BIT-ROWS.  One 64-bit word per 64 voxels along x, W[z][y][xw] with xw < ceil(nx / 64), bit i of word xw = voxel x = 64 xw + i:
// 16 MiB for a 512^3 volume beside its 2 GiB of voxels.  Bits beyond nx or outside the box are zero in every buffer, always.
//
// Pack (morph_pack_kernel): persistent workgroups of four wavefronts, one wavefront per word that meets the box, one lane per voxel;
// the word is ONE 64-bit ballot of in_box && v != 0.0f (vr_hist.h's membership rule: NaN is in, -0.0f is out).  |A'| and its bounding
// box come from the popcount and the first / last bit of the words.
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
// dst_contour and only where `combine` stores something; words that store nothing are skipped.  |R| and its box from the R words.
#pragma once

namespace vr {

// the bits of word xw whose voxels lie in [lo, hi) along x
__device__ __forceinline__ unsigned long long morph_xmask(int xw, int lo, int hi)
{
    const int a = max(lo - (xw << 6), 0), b = min(hi - (xw << 6), 64);  // bits [a, b)
    if (b <= a) return 0ull;
    const unsigned long long upto_b = b >= 64 ? ~0ull : ((1ull << b) - 1ull);
    return upto_b & ~((1ull << a) - 1ull);  // (a <= 63 here)
}

// folds one wavefront's word (its popcount, first and last bit, row and slice) into the words' count and bounding box; lane 0 alone
__device__ __forceinline__ void morph_fold(unsigned long long w, int xw, int y, int z, CountBox& n)
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

// word u of the box's words -> (xw, y, z): P.bw words per row from word P.bw0, rows and slices of the box
__device__ __forceinline__ void morph_box_word(const MorphParams& P, unsigned long long u, int& xw, int& y, int& z)
{
    const unsigned long long row = u / (unsigned)P.bw;
    xw = P.bw0 + (int)(u - row * (unsigned)P.bw);
    const unsigned rows = (unsigned)(P.hi[1] - P.lo[1]);
    const unsigned long long sl = row / rows;
    y = P.lo[1] + (int)(row - sl * rows);
    z = P.lo[2] + (int)sl;
}

__global__ __launch_bounds__(256) void morph_pack_kernel(const MorphParams P)
{
    const unsigned lane = threadIdx.x & 63u;
    const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const float* const src = reinterpret_cast<const float*>(P.src) + P.src_contour;
    CountBox n = CountBox::empty();  // (wave-uniform)
    const unsigned long long W = (unsigned long long)gridDim.x * 4ull;
    for (unsigned long long u = (unsigned long long)blockIdx.x * 4ull + wave; u < P.box_words; u += W) {
        int xw, y, z;
        morph_box_word(P, u, xw, y, z);
        const int x = (xw << 6) + (int)lane;
        bool in = false;
        if (x >= P.lo[0] && x < P.hi[0]) {  // (hi <= n; y and z are the box's)
            const size_t idx = ((size_t)z * (size_t)P.ny + (size_t)y) * (size_t)P.nx + (size_t)x;
            in = src[idx * 4u] != 0.0f;
        }
        const unsigned long long w = vr_ballot(in);
        if (lane == 0u) P.a[((size_t)z * (size_t)P.ny + (size_t)y) * (size_t)P.wx + (size_t)xw] = w;
        morph_fold(w, xw, y, z, n);
    }
    if (lane == 0u) report_count_box(&P.w->src, n.voxels, n.lo, n.hi);
}

// the source word (xw, y, z) of a dilation; COMP: of the box's complement
template <bool COMP>
__device__ __forceinline__ unsigned long long morph_src_word(const MorphParams& P, const unsigned long long* src, int xw, int y, int z)
{
    if (xw < 0 || xw >= P.wx || y < P.lo[1] || y >= P.hi[1] || z < P.lo[2] || z >= P.hi[2]) return 0ull;
    const unsigned long long w = src[((size_t)z * (size_t)P.ny + (size_t)y) * (size_t)P.wx + (size_t)xw];
    if constexpr (COMP) return ~w & morph_xmask(xw, P.lo[0], P.hi[0]);
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
    const unsigned long long box = morph_xmask(xw, P.lo[0], P.hi[0]);  // (the region's rows and slices are the box's)
    S.dst[((size_t)z * (size_t)P.ny + (size_t)y) * (size_t)P.wx + (size_t)xw] = (COMP ? ~c : c) & box;
}

__global__ __launch_bounds__(256) void morph_write_kernel(const MorphParams P)
{
    const unsigned lane = threadIdx.x & 63u;
    const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    float* const out = reinterpret_cast<float*>(P.dst) + P.dst_contour;
    CountBox n = CountBox::empty();  // (wave-uniform)
    const unsigned long long W = (unsigned long long)gridDim.x * 4ull;
    for (unsigned long long u = (unsigned long long)blockIdx.x * 4ull + wave; u < P.box_words; u += W) {
        int xw, y, z;
        morph_box_word(P, u, xw, y, z);
        const unsigned long long rw = P.r[((size_t)z * (size_t)P.ny + (size_t)y) * (size_t)P.wx + (size_t)xw];  // (zero outside the box)
        const unsigned long long box = morph_xmask(xw, P.lo[0], P.hi[0]);
        // the voxels that are stored: REPLACE all of the box (only R where the slot was created zeroed), OR and ANDNOT R, AND the rest
        unsigned long long st = rw;
        if (P.combine == VR_MORPH_REPLACE) st = P.fresh ? rw : box;
        else if (P.combine == VR_MORPH_AND) st = box & ~rw;
        if (st != 0ull) {
            const bool set = (rw >> lane) & 1ull;
            if ((st >> lane) & 1ull) {
                const size_t idx = ((size_t)z * (size_t)P.ny + (size_t)y) * (size_t)P.nx + (size_t)(xw << 6) + (size_t)lane;
                out[idx * 4u] = (set && P.combine <= VR_MORPH_OR) ? 1.0f : 0.0f;
            }
        }
        morph_fold(rw, xw, y, z, n);
    }
    if (lane == 0u) report_count_box(&P.w->result, n.voxels, n.lo, n.hi);
}

}  // namespace vr
