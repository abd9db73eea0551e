// vr_hist.h -- device histograms of one volume slot (vr_histogram_async, include/vr.h): how the values of one channel are distributed
// over a voxel box, overall (row 0) and inside each of the four contours of a mask volume (row 1 + c: mask component c != 0).
// Binning of a value v: t = v * scale (one f32 multiply), i = (int)t -- v_cvt_i32_f32: truncation toward zero, saturating, NaN -> 0
//  -- then CLAMP: bin = min(max(i, 0), bins - 1), or DROP: counted iff 0 <= i < bins, else one more in the row's `dropped`.
// Nothing can be fused, so vr_set_arithmetic plays no part: the kernel is compiled once, included by vr_api.hip alone.
//
// Launch shape: a fixed grid of kToolBlocks (vr_api_tools.h) persistent workgroups of four wavefronts.  The work is cut into BRICK UNITS, the 4 x 4 x 4
// voxel cubes of the volume's own brick grid that meet the box (so that units and range records line up); wavefront w of W takes the
// units w, w + W, ... with one lane per voxel of the unit (x fastest).  Lanes whose voxel lies outside the box -- a unit the box cuts,
// a side that is no multiple of 4 -- take no part: that is the whole partial path.
//
// Counts go into a private copy in the workgroup's LDS, u32[rows computed][bins], with ds_add_u32 (no return), and are flushed once per
// workgroup into the u64 outputs with global_atomic_add_x2.  The host bounds the voxels one workgroup can take below 2^32 (a u32
// count cannot wrap) and the copy by kHistLdsBytes; otherwise (HistParams::lds == 0) the same kernel adds straight into global memory.
//
// Contention.  A CT is more than half exact-zero air: a naive histogram sends more than half of its increments to one address.
// (a) Combining: per row, the lanes that hold the bin of the wavefront's first contributing lane are counted with one ballot and
//     that lane adds their number; the other contributing lanes add one each.  A wave-uniform unit costs one atomic instead of 64.
// (b) Exact settling (channel 3, no mask, a unit wholly inside the box): the unit's range record (min .a, max .a) of
//     brick_range_kernel (vr_prep.h) is read first.  If it is not the flagged (NaN, NaN) record and i(min) == i(max), the unit's 64
//     voxels are added to that bin -- or to `dropped` -- and nothing is loaded.  This is exact:
//       - for a fixed finite scale s, v -> fl(v * s) is monotone (non-decreasing for s >= 0, non-increasing for s <= 0: rounding is
//         monotone), and t -> (int)t is non-decreasing on the finite floats and the infinities a product can overflow to; so
//         v -> i(v) is monotone on the finite values a record that is not flagged spans;
//       - for s = +-inf, finite v: v < 0, v = +-0, v > 0 give -+inf, NaN, +-inf, that is INT_MIN / 0 / INT_MAX in this or the reverse
//         order: monotone again; for a NaN scale every product is NaN and i = 0, constant;
//       - a record spans the voxels [4 b, min(4 b + 4, n - 1)]^3, a superset of the unit's, and is flagged whenever one of them is
//         NaN or infinite; so every voxel of the unit has min <= v <= max, i(v) lies between i(min) and i(max), and equal ends pin it.
// vr_set_kernel_flavour(1) selects the plain form (PLAIN): no settling, no combining, every voxel of the box loaded.
//
// Masks: the mask voxel is loaded first, and the value only where a requested row needs it.  An unmasked channel-3 launch reads the
// 4-byte density plane when the layout has one (HistParams::val / val_stride address either).
#pragma once
#include "vr_device.h"  // the argument blocks, BoxUnits
#include "vr_shared.h"  // vr_ballot

namespace vr {

constexpr unsigned kHistLdsBytes = 65536;    // budget of the private copy (what a launch may ask for without opting in to more; two
                                             // workgroups' copies still share a CU's 160 KiB): rows computed * bins <= 16384

__device__ __forceinline__ int hist_index(float v, float scale)
{
    return (int)(v * scale);  // (v_cvt_i32_f32: toward zero, saturating, NaN -> 0)
}
// the bin of index i, -2 for a dropped voxel
__device__ __forceinline__ int hist_key(int i, int bins, int drop)
{
    if (drop) return (i >= 0 && i < bins) ? i : -2;
    return min(max(i, 0), bins - 1);
}

// n more in (row, bin): the private copy (its row `srow`) or the output
__device__ __forceinline__ void hist_add(const HistParams& H, unsigned* s_hist, unsigned srow, unsigned row, int bin, unsigned n)
{
    if (H.lds) atomicAdd(&s_hist[srow * H.bins + (unsigned)bin], n);
    else atomicAdd(&H.counts[(size_t)row * H.bins + (unsigned)bin], (unsigned long long)n);
}

template <bool PLAIN>
__global__ __launch_bounds__(256) void hist_kernel(const HistParams H)
{
    extern __shared__ unsigned s_hist[];
    const unsigned lane = threadIdx.x & 63u;
    const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const unsigned n_rows = (unsigned)__popc(H.rows);
    if (H.lds) {
        for (unsigned i = threadIdx.x; i < n_rows * H.bins; i += 256u) s_hist[i] = 0u;
        __syncthreads();
    }
    const int lx = (int)(lane & 3u), ly = (int)((lane >> 2) & 3u), lz = (int)(lane >> 4);
    unsigned long long vox[VR_HIST_ROWS] = {}, dropped[VR_HIST_ROWS] = {};  // per lane
    unsigned long long n_box = 0, n_load = 0, n_settled = 0;
    const unsigned W = gridDim.x * 4u, uxy = (unsigned)H.box.un[0] * (unsigned)H.box.un[1];
    for (unsigned u = blockIdx.x * 4u + wave; u < H.box.units; u += W) {
        const BrickUnit U = brick_unit(H.box, u, uxy);
        if constexpr (!PLAIN) {
            const bool whole = whole_unit<const BoxUnits&>(H.box, U);
            if (H.bricks && whole) {
                const float2 rec = H.bricks[((size_t)U.bz * (size_t)H.bny + (size_t)U.by) * (size_t)H.bnx + (size_t)U.bx];
                const int i0 = hist_index(rec.x, H.scale), i1 = hist_index(rec.y, H.scale);
                if (rec.x == rec.x && rec.y == rec.y && i0 == i1) {
                    const int k = hist_key(i0, (int)H.bins, H.drop);
                    if (lane == 0u) {
                        vox[0] += 64u;
                        n_box += 64u;
                        n_settled += 64u;
                        if (k >= 0) hist_add(H, s_hist, 0u, 0u, k, 64u);
                        else dropped[0] += 64u;
                    }
                    continue;
                }
            }
        }
        const int x = U.x0 + lx, y = U.y0 + ly, z = U.z0 + lz;
        const bool in = in_box(H.box, x, y, z);  // (hi <= n)
        const size_t idx = ((size_t)z * (size_t)H.ny + (size_t)y) * (size_t)H.nx + (size_t)x;
        unsigned sel = 0u;  // the rows this voxel belongs to
        if (in) {
            sel = H.rows & 1u;
            if (H.mask) {
                const float4 m = H.mask[idx];
                sel |= ((m.x != 0.0f ? 2u : 0u) | (m.y != 0.0f ? 4u : 0u) | (m.z != 0.0f ? 8u : 0u) | (m.w != 0.0f ? 16u : 0u)) & H.rows;
            }
        }
        int key = -1;
        if (sel != 0u) key = hist_key(hist_index(H.val[idx * (size_t)H.val_stride], H.scale), (int)H.bins, H.drop);
        n_box += in ? 1u : 0u;
        n_load += sel != 0u ? 1u : 0u;
        unsigned srow = 0u;
#pragma unroll
        for (unsigned r = 0; r < VR_HIST_ROWS; ++r) {
            if (!((H.rows >> r) & 1u)) continue;  // (wave-uniform)
            const int k = ((sel >> r) & 1u) ? key : -1;
            vox[r] += k != -1 ? 1u : 0u;
            dropped[r] += k == -2 ? 1u : 0u;
            if constexpr (PLAIN) {
                if (k >= 0) hist_add(H, s_hist, srow, r, k, 1u);
            } else {
                const unsigned long long act = vr_ballot(k >= 0);
                if (act != 0ull) {
                    const int leader = __ffsll((long long)act) - 1;
                    const int k0 = __builtin_amdgcn_readlane(k, leader);
                    const unsigned long long same = vr_ballot(k == k0);
                    if ((int)lane == leader) hist_add(H, s_hist, srow, r, k0, (unsigned)__popcll(same));
                    else if (k >= 0 && k != k0) hist_add(H, s_hist, srow, r, k, 1u);
                }
            }
            ++srow;
        }
    }
    if (H.lds) {
        __syncthreads();
        unsigned srow = 0u;
        for (unsigned r = 0; r < VR_HIST_ROWS; ++r) {
            if (!((H.rows >> r) & 1u)) continue;
            for (unsigned b = threadIdx.x; b < H.bins; b += 256u) {
                const unsigned n = s_hist[srow * H.bins + b];
                if (n != 0u) atomicAdd(&H.counts[(size_t)r * H.bins + b], (unsigned long long)n);
            }
            ++srow;
        }
    }
    // the wavefront's row sums and counters
#pragma unroll
    for (unsigned r = 0; r < VR_HIST_ROWS; ++r) {
        if (!((H.rows >> r) & 1u)) continue;
        const unsigned long long v = wave_sum_u64(vox[r]), d = wave_sum_u64(dropped[r]);
        if (lane == 0u) {
            if (v != 0ull) atomicAdd(&H.row_sums[2u * r], v);
            if (d != 0ull) atomicAdd(&H.row_sums[2u * r + 1u], d);
        }
    }
    n_box = wave_sum_u64(n_box);
    n_load = wave_sum_u64(n_load);
    n_settled = wave_sum_u64(n_settled);
    if (lane == 0u) {
        if (n_box != 0ull) atomicAdd(&H.stats[0], n_box);
        if (n_load != 0ull) atomicAdd(&H.stats[1], n_load);
        if (n_settled != 0ull) atomicAdd(&H.stats[2], n_settled);
    }
}

}  // namespace vr
