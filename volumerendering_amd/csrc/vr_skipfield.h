// vr_skipfield.h -- the build of the skip field: which empty-space bricks are active under the opacity table, their capped Chebyshev
// distance field, and the count, box and hull of the active bricks that the last pass reports to the host.  Integer work that exists
// once, in namespace vr; only the C ABI's translation unit (vr_api.hip) includes it.
#pragma once
#include "vr_device.h"
#include "vr_shared.h"  // vr_ballot

namespace vr {

// ---- brick distance field (rebuilt when the volume or the opacity table changes) --------------------------------
// first: 0 for active bricks, 255 for inert ones
__global__ void brick_active_kernel(const float2* __restrict__ rec, unsigned char* __restrict__ dist, int n, int use_rgb,
                                    int zero_prefix, int res_o)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float2 r = rec[i];
    bool inert;
    if (use_rgb && !(r.y <= 0.0f)) inert = false;
    else if (r.x <= 0.0f) inert = zero_prefix >= 0;
    else inert = floorf(r.x * (float)res_o - 0.5f) + 2.0f <= (float)zero_prefix;
    dist[i] = inert ? 255 : 0;
}
// Then the capped Chebyshev distance, separably: the L-infinity distance to the nearest active brick is
// d(p) = min_bz max(|dz|, min_by max(|dy|, min_bx |dx|)), so three 1-D passes -- x, y, z -- each h(i) = min_j max(|i - j|, f(j)),
// capped at kDistMax (no |i - j| >= kDistMax can matter) give min(distance, kDistMax) exactly, kDistMax where nothing is active.
constexpr int kDistHalo = kDistMax - 1;  // bricks on either side of a pass's tile that can lower a value below the cap
constexpr int kDistCols = 128;           // y / z passes: bricks along x per tile (128-byte rows)
constexpr int kDistRows = 64;            // ... and outputs along the pass's axis per tile

// x pass, in place: the input is 0 (active) or 255, the nearest active brick on either side of a brick a bit scan.  One wavefront per
// 64 bricks of a row, the activity of the 64 + 2 x 128 bricks around them as five ballots (the bytes it overwrites stay zero exactly
// where they were: the other wavefronts' ballots are unaffected).
__global__ void brick_dist_x_kernel(unsigned char* __restrict__ dist, int bnx, int rows)
{
    const int lane = (int)(threadIdx.x & 63u);
    const long long segs = (bnx + 63) >> 6, w = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (w >= segs * rows) return;  // (wave-uniform)
    const int x0 = (int)(w % segs) * 64;
    unsigned char* line = dist + (size_t)(w / segs) * (size_t)bnx;
    unsigned long long m[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const int x = x0 - 128 + 64 * k + lane;
        m[k] = vr_ballot(x >= 0 && x < bnx && line[x] == 0);
    }
    const unsigned long long le = m[2] & ((2ull << lane) - 1ull), ri = m[2] & ~((1ull << lane) - 1ull);  // (bits <= lane, >= lane)
    int d = kDistMax;
    if (le) d = lane - (63 - __clzll((long long)le));
    else if (m[1]) d = lane + 64 - (63 - __clzll((long long)m[1]));
    else if (m[0]) d = lane + 128 - (63 - __clzll((long long)m[0]));
    int e = kDistMax;
    if (ri) e = __ffsll((long long)ri) - 1 - lane;
    else if (m[3]) e = 64 + __ffsll((long long)m[3]) - 1 - lane;
    else if (m[4]) e = 128 + __ffsll((long long)m[4]) - 1 - lane;
    d = min(min(d, e), kDistMax);
    if (x0 + lane < bnx) line[x0 + lane] = (unsigned char)d;
}

// Active-brick count and box of a field (brick coordinates), accumulated by the z pass's workgroups: lo as 0x7fffffff - lo and hi as
// hi + 1 under atomicMax, so that all zeros is the empty state.  The last workgroup publishes it to pinned host memory, generation last,
// and zeroes it again for the next build.
// hlo / hhi: the same for n . b + kHullBias along the ten diagonal directions of the hull (vr_hull.h, kHullDir[3 ..]).
struct SkipSumDev {
    unsigned count, done;
    unsigned lo[3], hi[3];
    unsigned hlo[kHullDiag], hhi[kHullDiag];
};

// y and z passes (in -> out, never in place): a tile of kDistCols bricks along x by kDistRows along the pass's axis, with kDistHalo
// bricks of halo on either side, staged in LDS row by row (every global read a 128-byte row along x); each output scans outwards
// from its brick until the distance reaches the best value found.  Grid: (x tiles, axis tiles, `other` positions).  LAST (the z
// pass): the tile's active bricks are counted and boxed -- wavefront, then workgroup in LDS, then one atomic per value -- and the ten
// diagonals of their hull reduced the same way in a second round.
template <bool LAST>
__global__ void __launch_bounds__(256) brick_dist_axis_kernel(const unsigned char* __restrict__ in, unsigned char* __restrict__ out,
                                                               int bnx, int n_axis, size_t axis_stride, size_t other_stride,
                                                               SkipSumDev* __restrict__ sum, SkipSummary* __restrict__ host,
                                                               unsigned long long gen)
{
    constexpr int kTileRows = kDistRows + 2 * kDistHalo;
    __shared__ unsigned char tile[kTileRows][kDistCols];
    const int t = (int)threadIdx.x;
    const int x0 = (int)blockIdx.x * kDistCols, a0 = (int)blockIdx.y * kDistRows;
    const size_t base = (size_t)blockIdx.z * other_stride;
    for (int idx = t; idx < kTileRows * kDistCols; idx += 256) {
        const int r = idx / kDistCols, cx = idx % kDistCols, x = x0 + cx, a = a0 - kDistHalo + r;
        tile[r][cx] = (x < bnx && a >= 0 && a < n_axis) ? in[base + (size_t)a * axis_stride + (size_t)x] : (unsigned char)kDistMax;
    }
    __syncthreads();
    // no output of a column lies below the column's minimum over the tile: a column that holds it stops there (most columns of the y
    // pass through planes without an active brick are kDistMax throughout and scan nothing)
    __shared__ unsigned char col_min[kDistCols];
    if (t < kDistCols) {
        int m = kDistMax;
        for (int r = 0; r < kTileRows; ++r) m = min(m, (int)tile[r][t]);
        col_min[t] = (unsigned char)m;
    }
    __syncthreads();
    const int cx = t % kDistCols, x = x0 + cx, floor_c = col_min[cx];
    unsigned cnt = 0;
    int lo[3] = {0x7fffffff, 0x7fffffff, 0x7fffffff}, hi[3] = {-1, -1, -1};
    for (int i = t / kDistCols; i < kDistRows; i += 256 / kDistCols) {
        const int a = a0 + i;
        if (x >= bnx || a >= n_axis) continue;
        const int R = i + kDistHalo, reach = max(a, n_axis - 1 - a);
        int best = tile[R][cx];
        for (int k = 1; k < best && best > floor_c && k <= reach; ++k) best = min(best, max(k, (int)min(tile[R - k][cx], tile[R + k][cx])));
        out[base + (size_t)a * axis_stride + (size_t)x] = (unsigned char)best;
        if constexpr (LAST) {
            if (best == 0) {
                const int p[3] = {x, (int)blockIdx.z, a};  // (the z pass: axis z, `other` y)
                ++cnt;
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    lo[q] = min(lo[q], p[q]);
                    hi[q] = max(hi[q], p[q]);
                }
            }
        }
    }
    if constexpr (LAST) {
        const unsigned lane_cnt = cnt;  // this lane's own bricks, before the wavefront folds them
        const int lane_zlo = lo[2], lane_zhi = hi[2];
        for (int off = 32; off > 0; off >>= 1) {
            cnt += __shfl_down(cnt, off, 64);
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                lo[q] = min(lo[q], __shfl_down(lo[q], off, 64));
                hi[q] = max(hi[q], __shfl_down(hi[q], off, 64));
            }
        }
        __shared__ int red[4][7];
        __shared__ int hred[4][2 * kHullDiag];
        __shared__ bool last;
        const int wv = t >> 6;
        if ((t & 63) == 0) {
            red[wv][0] = (int)cnt;
            for (int q = 0; q < 3; ++q) {
                red[wv][1 + q] = lo[q];
                red[wv][4 + q] = hi[q];
            }
        }
        // The hull's diagonals, a second round: a lane's bricks share x and y (its column, the workgroup's `other` position), so the
        // extremes of n . b over them lie at the lane's lowest and highest z, which the box has: nothing per brick, and one direction
        // at a time through the wavefront (no more registers than the box took).
        for (int d = 0; d < kHullDiag; ++d) {
            const int nx = kHullDir[kHullAxes + d][0], ny = kHullDir[kHullAxes + d][1], nz = kHullDir[kHullAxes + d][2];
            int dlo = 0x7fffffff, dhi = -1;
            if (lane_cnt != 0) {
                const int xy = nx * x + ny * (int)blockIdx.z + kHullBias;
                dlo = xy + nz * (nz > 0 ? lane_zlo : lane_zhi);
                dhi = xy + nz * (nz > 0 ? lane_zhi : lane_zlo);
            }
            for (int off = 32; off > 0; off >>= 1) {
                dlo = min(dlo, __shfl_down(dlo, off, 64));
                dhi = max(dhi, __shfl_down(dhi, off, 64));
            }
            if ((t & 63) == 0) {
                hred[wv][d] = dlo;
                hred[wv][kHullDiag + d] = dhi;
            }
        }
        __syncthreads();
        if (t == 0) {
            for (int v = 1; v < 4; ++v) {
                red[0][0] += red[v][0];
                for (int q = 0; q < 3; ++q) {
                    red[0][1 + q] = min(red[0][1 + q], red[v][1 + q]);
                    red[0][4 + q] = max(red[0][4 + q], red[v][4 + q]);
                }
                for (int d = 0; d < kHullDiag; ++d) {
                    hred[0][d] = min(hred[0][d], hred[v][d]);
                    hred[0][kHullDiag + d] = max(hred[0][kHullDiag + d], hred[v][kHullDiag + d]);
                }
            }
            if (red[0][0] != 0) {
                atomicAdd(&sum->count, (unsigned)red[0][0]);
                for (int q = 0; q < 3; ++q) {
                    atomicMax(&sum->lo[q], 0x7fffffffu - (unsigned)red[0][1 + q]);
                    atomicMax(&sum->hi[q], (unsigned)(red[0][4 + q] + 1));
                }
                for (int d = 0; d < kHullDiag; ++d) {
                    atomicMax(&sum->hlo[d], 0x7fffffffu - (unsigned)hred[0][d]);
                    atomicMax(&sum->hhi[d], (unsigned)(hred[0][kHullDiag + d] + 1));
                }
            }
            __threadfence();
            last = atomicAdd(&sum->done, 1u) == gridDim.x * gridDim.y * gridDim.z - 1u;
        }
        __syncthreads();
        if (last && t == 0) {
            __threadfence();
            volatile SkipSumDev* v = sum;
            host->count = v->count;
            for (int q = 0; q < 3; ++q) {
                host->box[q] = (int)(0x7fffffffu - v->lo[q]);
                host->box[3 + q] = (int)v->hi[q] - 1;
            }
            for (int d = 0; d < kHullDiag; ++d) {  // (meaningless when the count is 0)
                host->hull_lo[d] = (int)(0x7fffffffu - v->hlo[d]) - kHullBias;
                host->hull_hi[d] = (int)v->hhi[d] - 1 - kHullBias;
            }
            __threadfence_system();
            host->gen = gen;  // (after the values: the host reads the generation first)
            v->count = 0;
            v->done = 0;
            for (int q = 0; q < 3; ++q) v->lo[q] = v->hi[q] = 0;
            for (int d = 0; d < kHullDiag; ++d) v->hlo[d] = v->hhi[d] = 0;
        }
    }
}

}  // namespace vr
