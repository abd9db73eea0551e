// vr_rank.h -- rank filters of a volume channel on the device (vr_volume_rank, include/vr.h): the value at position k of the ascending
// order of the N = (2 rx + 1)(2 ry + 1)(2 rz + 1) values around every voxel of a box -- median, grey erosion (k = 0), grey dilation
// (k = N - 1) -- of one component of a volume slot, written into one component of a volume slot.  A rank filter selects and never
// computes: values travel as their KEYS (filter_key of vr_filter.h: unsigned integers whose order is the header's total order on all
// 2^32 bit patterns) and every comparison is an UNSIGNED INTEGER one -- v_min_u32, v_max_u32, v_med3_u32, v_cmp_*_u32.  The f32 forms
// order neither +-0 nor NaNs this way and may quiet a signalling NaN.  The stored word is filter_unkey of the selected key: one of the
// input bit patterns, whatever the evaluation order.  vr_set_arithmetic plays no part; vr_api.hip alone includes this file.
//
// The selection kernels read the source (never the destination) and write a FIELD: one word per voxel of the box, x fastest.
// Indices beyond a FACE OF THE VOLUME read the face's voxel (VR_FILTER_CLAMP) or border_value (VR_FILTER_CONSTANT).
//
// Default form (rank_tile_kernel<PATH>): a workgroup of 256 lanes takes a tile of kRankTX x kRankTY x kRankTZ = 32 x 8 x 4 outputs of the
// box (x, y, z), four per lane (same x and y, the four z), and loads the tile grown by the radii -- at most 38 x 14 x 10 keys at r = 3 --
// once into LDS: 5320 words, 20.8 KiB of static LDS (the min / max path has a second buffer of 32 x 14 x 10 words: 38.3 KiB in all; four
// workgroups per CU of 160 KiB at the worst).  Lanes run along x: a wavefront reads two rows of 32 neighbouring words per instruction.
// Selection from there, one of three paths:
//   kRankMinMax  k = 0 or k = N - 1: three 1-D running minima (maxima) inside the tile, along x into the second buffer, along y back into
//                the first, along z into the field.  The minimum over a box is the minimum of minima: exact.  2 (rx + ry + rz) + 3 LDS
//                reads per output where the generic path takes up to 16 N.
//   kRankMed27   radii (1, 1, 1), k = 13: a network in registers that discards extremes as values arrive.  Of 15 keys neither the least
//                nor the greatest can be the 14th of 27; drop both, take the next key in, and so on with 14, 13, .. 4 keys; the median of
//                the last three is the answer.  The least and the greatest of s keys are moved to the ends with about 3 s / 2
//                compare-exchanges (one v_min_u32 and one v_max_u32 each): 150 exchanges as written -- 266 v_min_u32 / v_max_u32 in the
//                listing, where the halves nobody reads are gone -- and one v_med3_u32 per output, 27 LDS reads.
//   kRankGeneric everything else: a radix descent over the key, two bits per round from the top.  A round reads the N keys of the window
//                and counts those that share the prefix found so far and continue with 00, 01, 10; the three counts say which of the four
//                continuations holds position k.  Ties are counted like anything else.  A first pass takes the least and the greatest
//                key of the window: the rounds start at the highest pair of bits in which the two differ (at most 16 rounds of N LDS
//                reads), and a window of one value needs none.
// Plain form (vr_set_kernel_flavour(1), rank_plain_kernel): one lane per output voxel, the same radix descent with every key read
// straight from memory, whatever k and the radii: the on-device cross-check and the baseline.
// Write (rank_write_kernel): one lane per voxel of the box: one load of the field, one of the source's component at the same voxel (the
// `changed` count), one 4-byte store into component dst_channel; the counts and the least and greatest finite key are folded across
// the wavefront behind the loop and reported with one atomic each.  Every lane reads its own source voxel before it writes its own
// destination voxel and no other: the same slot with the same channel is the result of reading everything first.
//
// Voxel indices are 64-bit throughout.  No kernel waits for another workgroup: the launch boundaries are the visibility points.
#pragma once
#include "vr_filter.h"  // filter_key, filter_unkey

namespace vr {

constexpr int kRankMaxRadius = 3;                       // VR_RANK_MAX_RADIUS
constexpr int kRankTX = 32, kRankTY = 8, kRankTZ = 4;   // outputs of a tile along x, y, z: kRankTX * kRankTY lanes, kRankTZ outputs each
constexpr int kRankTileWords = (kRankTX + 2 * kRankMaxRadius) * (kRankTY + 2 * kRankMaxRadius) * (kRankTZ + 2 * kRankMaxRadius);
constexpr int kRankRowWords = kRankTX * (kRankTY + 2 * kRankMaxRadius) * (kRankTZ + 2 * kRankMaxRadius);  // after the minima along x
constexpr int kRankMinMax = 0, kRankMed27 = 1, kRankGeneric = 2;

// Kernel argument block of a selection: passed by value.
struct RankArgs {
    const unsigned* src;       // the source slot's x-fastest float4 voxels as words ...
    int channel;               // ... and the component read
    int n[3];                  // of the volume
    int lo[3], bn[3];          // the box: first voxel and extent per axis
    int r[3];                  // the radii
    unsigned k;                // the resolved rank, 0 .. N - 1
    int border;                // VR_FILTER_CLAMP / VR_FILTER_CONSTANT
    unsigned border_key;       // filter_key of border_value's bits
    unsigned* out;             // the field: one word per voxel of the box, x fastest
    unsigned tx, ty;           // tiles along x and y (default form)
    unsigned long long tiles;  // workgroup tiles of the default form
};

// The device words of one vr_volume_rank: set by the host before the write, read behind it.
struct RankWords {
    unsigned long long nonfinite, changed;
    unsigned lo_key, hi_key;   // filter_key of the least / greatest finite stored value (start: ~0u, 0u)
};
// Kernel argument block of the write.
struct RankWrite {
    const unsigned* field;     // one word per voxel of the box
    const unsigned* src;       // the source's voxels as words, src_channel added
    unsigned* dst;             // the destination's voxels as words, dst_channel added
    int nx, ny;                // of the volume
    int lo[3], n[3];           // the box
    RankWords* w;
};

// the key of voxel (x, y, z), which may lie beyond the volume's faces on any axis
__device__ __forceinline__ unsigned rank_load(const RankArgs& A, int x, int y, int z)
{
    const bool out = (unsigned)x >= (unsigned)A.n[0] || (unsigned)y >= (unsigned)A.n[1] || (unsigned)z >= (unsigned)A.n[2];
    if (out) {
        if (A.border != 0) return A.border_key;
        x = x < 0 ? 0 : (x >= A.n[0] ? A.n[0] - 1 : x);
        y = y < 0 ? 0 : (y >= A.n[1] ? A.n[1] - 1 : y);
        z = z < 0 ? 0 : (z >= A.n[2] ? A.n[2] - 1 : z);
    }
    const size_t i = (((size_t)z * (size_t)A.n[1] + (size_t)y) * (size_t)A.n[0] + (size_t)x) * 4u + (size_t)A.channel;
    // (device memory, said outright: a global load, not a flat one whose wait the LDS traffic would share)
    return filter_key(((const __attribute__((address_space(1))) unsigned*)A.src)[i]);
}

__device__ __forceinline__ unsigned rank_umin(unsigned a, unsigned b) { return a < b ? a : b; }
__device__ __forceinline__ unsigned rank_umax(unsigned a, unsigned b) { return a > b ? a : b; }

// The key at position k of the ascending order of the keys a window holds.  each(count) calls count(key) for every key of the window,
// once per round, in any order.
template <typename Each>
__device__ __forceinline__ unsigned rank_descend(unsigned k, Each each)
{
    // the least and the greatest key of the window: every key shares the bits above the highest one in which the two differ, so the
    // descent starts at the pair of bits that holds it -- and a window of one value (air, a constant region) is done here
    unsigned lo = ~0u, hi = 0u;
    each([&](unsigned key) {
        lo = rank_umin(lo, key);
        hi = rank_umax(hi, key);
    });
    if (lo == hi) return lo;
    const int top = (31 - __clz((int)(lo ^ hi))) & ~1;
    unsigned prefix = top == 30 ? 0u : (lo >> (top + 2)) << (top + 2);
    for (int shift = top; shift >= 0; shift -= 2) {
        unsigned c0 = 0u, c1 = 0u, c2 = 0u;
        // q < 4 iff the key shares the bits above `shift` with the prefix (whose bits from `shift` down are still 0): then q is its
        // next two bits
        each([&](unsigned key) {
            const unsigned q = (key ^ prefix) >> shift;
            c0 += q == 0u ? 1u : 0u;
            c1 += q == 1u ? 1u : 0u;
            c2 += q == 2u ? 1u : 0u;
        });
        unsigned digit = 3u, below = c0 + c1 + c2;
        if (k < c0) digit = 0u, below = 0u;
        else if (k < c0 + c1) digit = 1u, below = c0;
        else if (k < c0 + c1 + c2) digit = 2u, below = c0 + c1;
        k -= below;
        prefix |= digit << shift;
    }
    return prefix;
}

// compare-exchange: the lesser key into a, the greater into b
__device__ __forceinline__ void rank_cx(unsigned& a, unsigned& b)
{
    const unsigned l = rank_umin(a, b);
    b = rank_umax(a, b);
    a = l;
}

// moves the least of v[0 .. S - 1] to v[0] and the greatest to v[S - 1]; the rest stays the same multiset
template <int S>
__device__ __forceinline__ void rank_ends(unsigned* v)
{
#pragma unroll
    for (int i = 0; i < S / 2; ++i) rank_cx(v[i], v[S - 1 - i]);  // the least is now in v[0 .. (S - 1) / 2], the greatest in v[S / 2 .. S - 1]
#pragma unroll
    for (int i = 1; i <= (S - 1) / 2; ++i) rank_cx(v[0], v[i]);
#pragma unroll
    for (int i = S / 2; i < S - 1; ++i) rank_cx(v[i], v[S - 1]);
}

// one step of the network: of the S keys v[0 .. S - 1] the least and the greatest leave, `next` arrives: S - 1 keys in v[0 .. S - 2]
template <int S>
__device__ __forceinline__ void rank_drop(unsigned* v, unsigned next)
{
    rank_ends<S>(v);
    v[0] = v[S - 2];  // (v[S - 1], the greatest, leaves; v[0], the least, is overwritten)
    v[S - 2] = next;
}

// the median of 27 keys: in(i) is key i
template <typename In>
__device__ __forceinline__ unsigned rank_med27(In in)
{
    unsigned v[15];
#pragma unroll
    for (int i = 0; i < 15; ++i) v[i] = in(i);
    rank_drop<15>(v, in(15));
    rank_drop<14>(v, in(16));
    rank_drop<13>(v, in(17));
    rank_drop<12>(v, in(18));
    rank_drop<11>(v, in(19));
    rank_drop<10>(v, in(20));
    rank_drop<9>(v, in(21));
    rank_drop<8>(v, in(22));
    rank_drop<7>(v, in(23));
    rank_drop<6>(v, in(24));
    rank_drop<5>(v, in(25));
    rank_drop<4>(v, in(26));
    // the median of three, as unsigned integers
    return rank_umax(rank_umin(v[0], v[1]), rank_umin(rank_umax(v[0], v[1]), v[2]));
}

template <int PATH, bool MAX>
__global__ __launch_bounds__(256) void rank_tile_kernel(const RankArgs A)
{
    __shared__ unsigned tile[kRankTileWords];
    __shared__ unsigned rows[PATH == kRankMinMax ? kRankRowWords : 1];
    const int tid = (int)threadIdx.x, lx = tid & (kRankTX - 1), ly = tid >> 5;
    const int rx = A.r[0], ry = A.r[1], rz = A.r[2];
    const int ex = kRankTX + 2 * rx, ey = kRankTY + 2 * ry, ez = kRankTZ + 2 * rz, total = ex * ey * ez;
    for (unsigned long long u = blockIdx.x; u < A.tiles; u += gridDim.x) {
        const unsigned long long g = u / A.tx, h = g / A.ty;
        const int x0 = (int)(u - g * A.tx) * kRankTX, y0 = (int)(g - h * A.ty) * kRankTY, z0 = (int)h * kRankTZ;  // within the box
        for (int i = tid; i < total; i += 256) {
            const int row = i / ex, iz = row / ey;
            tile[i] = rank_load(A, A.lo[0] + x0 - rx + (i - row * ex), A.lo[1] + y0 - ry + (row - iz * ey), A.lo[2] + z0 - rz + iz);
        }
        __syncthreads();
        const int x = x0 + lx, y = y0 + ly;
        const bool in_xy = x < A.bn[0] && y < A.bn[1];
        if (PATH == kRankMinMax) {
            for (int i = tid; i < kRankTX * ey * ez; i += 256) {  // along x: every row of the grown tile
                const unsigned* const p = tile + (i >> 5) * ex + (i & 31);
                unsigned m = p[0];
                for (int t = 1; t <= 2 * rx; ++t) m = MAX ? rank_umax(m, p[t]) : rank_umin(m, p[t]);
                rows[i] = m;
            }
            __syncthreads();
            for (int i = tid; i < kRankTX * kRankTY * ez; i += 256) {  // along y: (x, y) of the tile for every z of the grown tile
                const int iz = i >> 8;
                const unsigned* const p = rows + (iz * ey + ((i >> 5) & 7)) * kRankTX + (i & 31);
                unsigned m = p[0];
                for (int t = 1; t <= 2 * ry; ++t) m = MAX ? rank_umax(m, p[t * kRankTX]) : rank_umin(m, p[t * kRankTX]);
                tile[i] = m;  // (the minima along x have all been taken: the first buffer is free)
            }
            __syncthreads();
        }
#pragma unroll
        for (int q = 0; q < kRankTZ; ++q) {
            const int z = z0 + q;
            if (!in_xy || z >= A.bn[2]) continue;
            unsigned key;
            if (PATH == kRankMinMax) {
                const unsigned* const p = tile + (q * kRankTY + ly) * kRankTX + lx;
                key = p[0];
                for (int t = 1; t <= 2 * rz; ++t) key = MAX ? rank_umax(key, p[t * kRankTX * kRankTY]) : rank_umin(key, p[t * kRankTX * kRankTY]);
            } else if (PATH == kRankMed27) {
                const unsigned* const p = tile + (q * ey + ly) * ex + lx;
                key = rank_med27([&](int i) { return p[((i / 9) * ey + (i / 3) % 3) * ex + i % 3]; });
            } else {
                const unsigned* const p = tile + (q * ey + ly) * ex + lx;
                key = rank_descend(A.k, [&](auto count) {
                    for (int dz = 0; dz <= 2 * rz; ++dz)
                        for (int dy = 0; dy <= 2 * ry; ++dy) {
                            const unsigned* const line = p + (dz * ey + dy) * ex;
                            for (int dx = 0; dx <= 2 * rx; ++dx) count(line[dx]);
                        }
                });
            }
            A.out[((size_t)z * (size_t)A.bn[1] + (size_t)y) * (size_t)A.bn[0] + (size_t)x] = filter_unkey(key);
        }
        __syncthreads();  // (the next tile overwrites this one)
    }
}

__global__ __launch_bounds__(256) void rank_plain_kernel(const RankArgs A)
{
    const unsigned long long n = (unsigned long long)A.bn[0] * (unsigned long long)A.bn[1] * (unsigned long long)A.bn[2];
    const unsigned long long step = (unsigned long long)gridDim.x * 256ull;
    const int rx = A.r[0], ry = A.r[1], rz = A.r[2];
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x; i < n; i += step) {
        const unsigned long long row = i / (unsigned)A.bn[0], sl = row / (unsigned)A.bn[1];
        const int x = A.lo[0] + (int)(i - row * (unsigned)A.bn[0]), y = A.lo[1] + (int)(row - sl * (unsigned)A.bn[1]), z = A.lo[2] + (int)sl;
        const unsigned key = rank_descend(A.k, [&](auto count) {
            for (int dz = -rz; dz <= rz; ++dz)
                for (int dy = -ry; dy <= ry; ++dy)
                    for (int dx = -rx; dx <= rx; ++dx) count(rank_load(A, x + dx, y + dy, z + dz));
        });
        A.out[i] = filter_unkey(key);
    }
}

__global__ __launch_bounds__(256) void rank_write_kernel(const RankWrite W)
{
    const unsigned long long n = (unsigned long long)W.n[0] * (unsigned long long)W.n[1] * (unsigned long long)W.n[2];
    const unsigned long long step = (unsigned long long)gridDim.x * 256ull;
    unsigned long long nonfinite = 0ull, changed = 0ull;
    unsigned lo = ~0u, hi = 0u;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x; i < n; i += step) {
        const unsigned long long row = i / (unsigned)W.n[0], sl = row / (unsigned)W.n[1];
        const int x = W.lo[0] + (int)(i - row * (unsigned)W.n[0]), y = W.lo[1] + (int)(row - sl * (unsigned)W.n[1]), z = W.lo[2] + (int)sl;
        const size_t at = (((size_t)z * (size_t)W.ny + (size_t)y) * (size_t)W.nx + (size_t)x) * 4u;
        const unsigned bits = W.field[i];
        if (W.src[at] != bits) ++changed;  // (read before the store below, which may be to the same word)
        W.dst[at] = bits;
        if ((bits & 0x7f800000u) == 0x7f800000u) ++nonfinite;
        else {
            const unsigned k = filter_key(bits);
            lo = k < lo ? k : lo;
            hi = k > hi ? k : hi;
        }
    }
    nonfinite = wave_sum_u64(nonfinite);  // (behind the loop: every lane takes part in the folds)
    changed = wave_sum_u64(changed);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned l = (unsigned)__shfl_down((int)lo, off, 64), h = (unsigned)__shfl_down((int)hi, off, 64);
        lo = l < lo ? l : lo;
        hi = h > hi ? h : hi;
    }
    if ((threadIdx.x & 63u) == 0u) {
        if (nonfinite != 0ull) atomicAdd(&W.w->nonfinite, nonfinite);
        if (changed != 0ull) atomicAdd(&W.w->changed, changed);
        if (lo <= hi) {  // (some finite value)
            atomicMin(&W.w->lo_key, lo);
            atomicMax(&W.w->hi_key, hi);
        }
    }
}

}  // namespace vr
