// vr_grow.h -- region growing from seed voxels into one contour of a mask volume (vr_segment_grow, include/vr.h): the voxels of a box
// whose channel value lies in [lo, hi] and that are connected to a seed through such voxels, 6- or 26-connected.
// Nothing can be fused, so vr_set_arithmetic plays no part: the kernels are compiled once, included by vr_api.hip alone.
//
// State: BIT-BRICKS.  Every 4 x 4 x 4 brick of the volume's own brick grid has two 64-bit words, Q (the voxel qualifies and lies in the
// box) and R (the voxel is reached), bit x + 4 y + 16 z: 16 B per 64 voxels, 32 MiB for a 512^3 volume beside its 2 GiB of voxels.  Bits
// of voxels outside the volume or the box are never set in Q, and R is a subset of Q throughout: adjacency cannot leave the box.
//
// Classify (grow_classify_kernel): the walk of vr_units.h -- persistent workgroups of four wavefronts, one wavefront per brick
// unit that meets the box, one lane per voxel -- and Q is one 64-bit ballot of in_box && v >= lo && v <= hi.  Exact settling (channel
// 3, a unit wholly inside the box, a range record (min .a, max .a) of brick_range_kernel that is not the flagged (NaN, NaN) one):
//     max < lo || min > hi    ->  Q = 0         min >= lo && max <= hi  ->  Q = all ones
// and nothing is loaded.  This is exact: a record spans the voxels [4 b, min(4 b + 4, n - 1)]^3, a superset of the unit's, and is
// flagged whenever one of them is NaN, infinite or above 2^125 in magnitude; so every voxel v of the unit is a number with
// min <= v <= max, and the comparisons are those of the voxel test itself (f32 compares are exact and transitive on numbers):
// max < lo gives v < lo, min > hi gives v > hi, min >= lo && max <= hi gives lo <= v <= hi.  A NaN bound fails all four and the unit is
// loaded, where every voxel fails.  vr_set_kernel_flavour(1) selects the plain form: no settling, every voxel of the box loaded.
//
// Seed (grow_seed_kernel): one lane per seed ORs its bit into R if it is in Q, and queues the brick for round 1.
//
// Propagate (grow_round_kernel), one launch per round, one wavefront per brick: lanes 0 .. 26 load the R words of the brick's
// neighbours (6 or 26 of them) and turn each into the bits it reaches in THIS brick (grow_cross: the facing layer, moved across the
// border and, for 26 neighbours, dilated along the axes the two bricks share); the wavefront ORs them into `incoming`, and the brick's
// local fixpoint r <- Q & (r | incoming | dilate(r)) is plain 64-bit integer arithmetic:
//     x: shifts by 1 with the x = 3 / x = 0 columns masked out, so that rows do not wrap; y: by 4 with the y rows masked; z: by 16;
//     26 neighbours: the three axis dilations composed (the Chebyshev ball is separable).
// Two forms, bit-identical in everything but the number of rounds:
//   frontier (default): round k works on a list of bricks.  A brick whose R changed stores it and queues every neighbour that has a Q
//     bit it could gain for round k + 1; a per-brick round stamp (an atomic exchange) drops duplicates, the list's length is a
//     device-scope counter.  Round 1 queues whether R changed or not (the seeds' bits are news to the neighbours).
//   sweep (vr_set_kernel_flavour(1)): every brick with Q != 0 in every round, one "changed" word.
// A brick has a single writer per round; a neighbour's R read within a launch may be stale (per-XCD L2s are not coherent), which is
// harmless: R only grows, and the brick that changed queues its neighbours for the next round (the sweep visits them anyway).  The
// launch boundary makes a round visible to the next.  No kernel waits for another workgroup.  A round whose input word is zero returns
// at once; the host enqueues rounds in batches and reads the words behind each batch.
//
// Write (grow_write_kernel): component `contour` of the mask voxels with one 4-byte vector store per voxel (the other three components
// are never read or written), only in bricks with R != 0 unless zeros must be stored; |R| and its box from popcounts of the R words.
#pragma once
#include "vr_device.h"  // the argument blocks, BoxUnits
#include "vr_shared.h"  // vr_ballot

namespace vr {

constexpr unsigned long long kGrowX0 = 0x1111111111111111ull, kGrowX3 = 0x8888888888888888ull;  // the x = 0 / x = 3 columns
constexpr unsigned long long kGrowY0 = 0x000F000F000F000Full, kGrowY3 = 0xF000F000F000F000ull;  // the y = 0 / y = 3 rows
constexpr unsigned long long kGrowZ0 = 0x000000000000FFFFull, kGrowZ3 = 0xFFFF000000000000ull;  // the z = 0 / z = 3 slices

__device__ __forceinline__ unsigned long long grow_dilate_x(unsigned long long r) { return r | ((r & ~kGrowX3) << 1) | ((r & ~kGrowX0) >> 1); }
__device__ __forceinline__ unsigned long long grow_dilate_y(unsigned long long r) { return r | ((r & ~kGrowY3) << 4) | ((r & ~kGrowY0) >> 4); }
__device__ __forceinline__ unsigned long long grow_dilate_z(unsigned long long r) { return r | (r << 16) | (r >> 16); }

// r and its neighbours inside the brick
__device__ __forceinline__ unsigned long long grow_dilate(unsigned long long r, int all)
{
    if (all) return grow_dilate_z(grow_dilate_y(grow_dilate_x(r)));
    return grow_dilate_x(r) | grow_dilate_y(r) | grow_dilate_z(r);
}

// The voxels of the brick at the origin that are neighbours of a set voxel of word w of the brick at offset (dx, dy, dz), each -1 .. 1 and
// not all zero (6 neighbours: exactly one is not zero).  Per axis: across the border the facing layer lands on the layer it touches;
// along a shared axis the bits stay (6) or spread by one (26).
__device__ __forceinline__ unsigned long long grow_cross(unsigned long long w, int dx, int dy, int dz, int all)
{
    if (dx > 0) w = (w & kGrowX0) << 3;
    else if (dx < 0) w = (w & kGrowX3) >> 3;
    else if (all) w = grow_dilate_x(w);
    if (dy > 0) w = (w & kGrowY0) << 12;
    else if (dy < 0) w = (w & kGrowY3) >> 12;
    else if (all) w = grow_dilate_y(w);
    if (dz > 0) w = (w & kGrowZ0) << 48;
    else if (dz < 0) w = (w & kGrowZ3) >> 48;
    else if (all) w = grow_dilate_z(w);
    return w;
}

__device__ __forceinline__ unsigned long long grow_wave_or(unsigned long long v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v |= __shfl_xor(v, off, 64);  // (every lane takes part)
    return v;
}

template <bool PLAIN>
__global__ __launch_bounds__(256) void grow_classify_kernel(const GrowParams P)
{
    const unsigned lane = threadIdx.x & 63u;
    const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lx = (int)(lane & 3u), ly = (int)((lane >> 2) & 3u), lz = (int)(lane >> 4);
    unsigned long long n_box = 0, n_load = 0, n_settled = 0;  // per lane
    const unsigned W = gridDim.x * 4u, uxy = (unsigned)P.box.un[0] * (unsigned)P.box.un[1];
    for (unsigned u = blockIdx.x * 4u + wave; u < P.box.units; u += W) {
        const BrickUnit U = brick_unit(P.box, u, uxy);
        const size_t b = ((size_t)U.bz * (size_t)P.bny + (size_t)U.by) * (size_t)P.bnx + (size_t)U.bx;  // (< n_bricks: the unit meets the volume)
        if constexpr (!PLAIN) {
            const bool whole = whole_unit<BoxUnits>(P.box, U);
            if (P.bricks && whole) {
                const float2 rec = P.bricks[b];
                const bool none = rec.y < P.vlo || rec.x > P.vhi, every = rec.x >= P.vlo && rec.y <= P.vhi;  // (the flagged record fails both)
                if (none || every) {
                    if (lane == 0u) {
                        P.q[b] = every ? ~0ull : 0ull;
                        n_box += 64u;
                        n_settled += 64u;
                    }
                    continue;
                }
            }
        }
        const int x = U.x0 + lx, y = U.y0 + ly, z = U.z0 + lz;
        const bool in = in_box(P.box, x, y, z);  // (hi <= n)
        bool ok = false;
        if (in) {
            const size_t idx = ((size_t)z * (size_t)P.ny + (size_t)y) * (size_t)P.nx + (size_t)x;
            const float v = P.val[idx * (size_t)P.val_stride];
            ok = v >= P.vlo && v <= P.vhi;
        }
        const unsigned long long qw = vr_ballot(ok);
        if (lane == 0u) P.q[b] = qw;
        n_box += in ? 1u : 0u;
        n_load += in ? 1u : 0u;
    }
    n_box = wave_sum_u64(n_box);
    n_load = wave_sum_u64(n_load);
    n_settled = wave_sum_u64(n_settled);
    if (lane == 0u) {
        if (n_box != 0ull) atomicAdd(&P.w->stats[0], n_box);
        if (n_load != 0ull) atomicAdd(&P.w->stats[1], n_load);
        if (n_settled != 0ull) atomicAdd(&P.w->stats[2], n_settled);
    }
}

// One lane per seed: its bit into R if it lies in the box and in Q; the brick is queued for round 1 once (the sweep takes the count
// alone: "there is something to do").
template <bool SWEEP>
__global__ __launch_bounds__(64) void grow_seed_kernel(const GrowParams P, const GrowSeeds S)
{
    const unsigned i = threadIdx.x;
    if (i >= S.n) return;
    const int x = S.xyz[i][0], y = S.xyz[i][1], z = S.xyz[i][2];
    if (!in_box(P.box, x, y, z)) return;
    const unsigned b = ((unsigned)(z >> 2) * (unsigned)P.bny + (unsigned)(y >> 2)) * (unsigned)P.bnx + (unsigned)(x >> 2);
    const unsigned long long bit = 1ull << ((x & 3) + 4 * (y & 3) + 16 * (z & 3));
    if (b >= P.n_bricks || !(P.q[b] & bit)) return;
    atomicOr(&P.r[b], bit);
    if (atomicExch(&P.stamp[b], 1u) != 1u) {
        const unsigned at = atomicAdd(&P.w->cnt[1], 1u);
        if (!SWEEP && at < P.n_bricks) P.list[1][at] = b;
    }
}

template <bool SWEEP>
__global__ __launch_bounds__(256) void grow_round_kernel(const GrowParams P)
{
    const unsigned k = P.round;
    const unsigned n_in = P.w->cnt[k % 3u];  // (written by the launch before this one)
    if (blockIdx.x == 0u && threadIdx.x == 0u) {
        P.w->cnt[(k + 2u) % 3u] = 0u;  // the next round's output word: nobody reads or writes it during this launch
        if (n_in != 0u) P.w->rounds = k;
    }
    if (n_in == 0u) return;
    unsigned* const n_out = &P.w->cnt[(k + 1u) % 3u];
    const unsigned lane = threadIdx.x & 63u;
    const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int dx = (int)(lane % 3u) - 1, dy = (int)((lane / 3u) % 3u) - 1, dz = (int)(lane / 9u) - 1;  // (lanes 0 .. 26)
    const int nz_axes = (dx != 0) + (dy != 0) + (dz != 0);
    const bool nb_lane = lane < 27u && nz_axes != 0 && (P.all || nz_axes == 1);
    const unsigned* const list_in = P.list[k & 1u];
    unsigned* const list_out = P.list[(k + 1u) & 1u];
    const unsigned W = gridDim.x * 4u, bxy = (unsigned)P.bnx * (unsigned)P.bny;
    const unsigned n_items = SWEEP ? P.n_bricks : (n_in < P.n_bricks ? n_in : P.n_bricks);
    for (unsigned i = blockIdx.x * 4u + wave; i < n_items; i += W) {
        unsigned b = i;
        if constexpr (!SWEEP) {
            b = list_in[i];
            if (b >= P.n_bricks) continue;
        }
        const unsigned long long qw = P.q[b];
        if (qw == 0ull) continue;  // (wave-uniform; the frontier never queues such a brick)
        const unsigned long long r_old = P.r[b];
        const int bz = (int)(b / bxy), brem = (int)(b - (unsigned)bz * bxy), by = brem / P.bnx, bx = brem - by * P.bnx;
        const int ax = bx + dx, ay = by + dy, az = bz + dz;
        const bool have = nb_lane && ax >= 0 && ax < P.bnx && ay >= 0 && ay < P.bny && az >= 0 && az < P.bnz;
        const unsigned nb = have ? ((unsigned)az * (unsigned)P.bny + (unsigned)ay) * (unsigned)P.bnx + (unsigned)ax : 0u;
        const unsigned long long rn = have ? P.r[nb] : 0ull;
        const unsigned long long incoming = grow_wave_or(have ? grow_cross(rn, dx, dy, dz, P.all) : 0ull);
        unsigned long long r_new = (r_old | incoming) & qw;
        for (int it = 0; it < 64; ++it) {  // (a brick's longest path has 64 voxels)
            const unsigned long long next = qw & grow_dilate(r_new, P.all);
            if (next == r_new) break;
            r_new = next;
        }
        const bool changed = r_new != r_old;
        if (changed && lane == 0u) P.r[b] = r_new;
        if constexpr (SWEEP) {
            if (changed && lane == 0u) atomicOr(n_out, 1u);
        } else {
            if ((changed || k == 1u) && have) {
                // what this brick reaches in the neighbour (seen from there, this brick lies at the opposite offset)
                const unsigned long long gain = grow_cross(r_new, -dx, -dy, -dz, P.all) & P.q[nb] & ~rn;
                if (gain != 0ull && atomicExch(&P.stamp[nb], k + 1u) != k + 1u) {
                    const unsigned at = atomicAdd(n_out, 1u);
                    if (at < P.n_bricks) list_out[at] = nb;  // (a brick is queued once per round: at < n_bricks)
                }
            }
        }
    }
}

// occupancy of a 64-bit brick word per axis: bit i of the result = some voxel with that coordinate equal to i is set
__device__ __forceinline__ unsigned grow_occ_x(unsigned long long r)
{
    unsigned m = (unsigned)(r | (r >> 16) | (r >> 32) | (r >> 48)) & 0xFFFFu;
    return (m | (m >> 4) | (m >> 8) | (m >> 12)) & 0xFu;
}
__device__ __forceinline__ unsigned grow_occ_y(unsigned long long r)
{
    const unsigned m = (unsigned)(r | (r >> 16) | (r >> 32) | (r >> 48)) & 0xFFFFu;
    return ((m & 0x000Fu) ? 1u : 0u) | ((m & 0x00F0u) ? 2u : 0u) | ((m & 0x0F00u) ? 4u : 0u) | ((m & 0xF000u) ? 8u : 0u);
}
__device__ __forceinline__ unsigned grow_occ_z(unsigned long long r)
{
    return ((r & kGrowZ0) ? 1u : 0u) | ((r & (kGrowZ0 << 16)) ? 2u : 0u) | ((r & (kGrowZ0 << 32)) ? 4u : 0u) | ((r & kGrowZ3) ? 8u : 0u);
}

__global__ __launch_bounds__(256) void grow_write_kernel(const GrowParams P)
{
    const unsigned lane = threadIdx.x & 63u;
    const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lx = (int)(lane & 3u), ly = (int)((lane >> 2) & 3u), lz = (int)(lane >> 4);
    float* const out = reinterpret_cast<float*>(P.mask) + P.contour;
    CountBox n = CountBox::empty();  // (wave-uniform)
    const unsigned W = gridDim.x * 4u, bxy = (unsigned)P.bnx * (unsigned)P.bny;
    for (unsigned b = blockIdx.x * 4u + wave; b < P.n_bricks; b += W) {
        const unsigned long long rw = P.r[b];
        if (rw == 0ull && !P.write_zeros) continue;
        const int bz = (int)(b / bxy), brem = (int)(b - (unsigned)bz * bxy), by = brem / P.bnx, bx = brem - by * P.bnx;
        const int x = (bx << 2) + lx, y = (by << 2) + ly, z = (bz << 2) + lz;
        const bool set = (rw >> lane) & 1ull;
        if (x < P.nx && y < P.ny && z < P.nz && (set || P.write_zeros)) {
            const size_t idx = ((size_t)z * (size_t)P.ny + (size_t)y) * (size_t)P.nx + (size_t)x;
            out[idx * 4u] = set ? 1.0f : 0.0f;
        }
        if (rw != 0ull) {
            n.voxels += (unsigned long long)__popcll(rw);
            const unsigned ox = grow_occ_x(rw), oy = grow_occ_y(rw), oz = grow_occ_z(rw);
            n.lo[0] = min(n.lo[0], (bx << 2) + __ffs((int)ox) - 1);
            n.lo[1] = min(n.lo[1], (by << 2) + __ffs((int)oy) - 1);
            n.lo[2] = min(n.lo[2], (bz << 2) + __ffs((int)oz) - 1);
            n.hi[0] = max(n.hi[0], (bx << 2) + 32 - __clz((int)ox));
            n.hi[1] = max(n.hi[1], (by << 2) + 32 - __clz((int)oy));
            n.hi[2] = max(n.hi[2], (bz << 2) + 32 - __clz((int)oz));
        }
    }
    if (lane == 0u) report_count_box(&P.w->reached, n.voxels, n.lo, n.hi);
}

}  // namespace vr
