// vr_filter.h -- separable filters of a volume channel on the device (vr_volume_filter, include/vr.h): up to three 1-D correlations, along
// x, then y, then z, of one component of a volume slot, restricted to a box, written as f32 into one component of a volume slot.  The
// arithmetic is the header's and it is FUSED ALWAYS: one rounded product for the first tap, one explicit fmaf per further tap, in
// ascending tap order.  vr_set_arithmetic plays no part (the unit is compiled with -ffp-contract=off, so nothing else is contracted, and
// an fmaf is an fmaf under either flag), which is why these kernels exist once, included by vr_api.hip alone.
//
// A FIELD is one f32 per voxel of a REGION of the volume, x fastest (FilterView with stride 1); the source is the same view with stride 4
// over the whole volume: component src_channel of the x-fastest float4 array.  Pass k along axis a computes the region
// "the box, grown on every later axis that has a pass by that axis' radius, clipped to the volume" from the field of pass k - 1 (the
// first one from the source), so every index a pass reads along its axis after clamping lies in its input's region.  Indices beyond a
// FACE OF THE VOLUME read the face's voxel (VR_FILTER_CLAMP) or border_value (VR_FILTER_CONSTANT), in every pass.
//
// Default form, every input value loaded once per workgroup tile (plus the halo) into LDS, the taps applied from LDS:
//   x pass (filter_x_kernel): a workgroup of 256 lanes takes a run of kFilterRun = 256 outputs of a row; the tile is the run + 2 r
//     values, at most 320 floats.  Lane i reads tile[i + t]: neighbouring lanes, neighbouring banks.  It takes the same run of
//     kFilterRows = 8 rows at a time, so that eight loads per lane are in flight between two barriers, not one (one row at a time reached
//     2.9 TB/s on the 512^3 CT), and a weight is fetched once for eight multiply-adds.
//   y and z passes (filter_line_kernel): a workgroup takes 64 consecutive x by kFilterT outputs along the axis; the tile is
//     (kFilterT + 2 r) rows of 64 floats.  Lanes run along x: a wavefront loads and stores one run of 256 bytes (of 1 KiB from the
//     float4 source) and reads one LDS row, 64 neighbouring banks, per instruction.  Each of the four wavefronts keeps kFilterT / 4
//     accumulators per lane, so a weight is fetched once for 16 multiply-adds, and loads its rows of the tile kFilterBatch = 8 at a
//     time into registers before it stores them, so that they are in flight together.
//     kFilterT = 64: the values loaded per value stored are (T + 2 r) / T -- 1.125 at r = 4 (sigma = 1 voxel), 2 at r = 32; T = 32 would
//     load 1.25 and 3, T = 128 needs 48 KiB of LDS at r = 32 and 32 accumulators per lane for a gain of 6 % at r = 4.  The tile is
//     dynamic shared memory of (T + 2 r) * 256 bytes: 18 KiB at r = 4, 32 KiB at r = 32 -- five workgroups per CU at the worst.
//   The weights travel in the parameter struct and are indexed by the (wave-uniform) tap: scalar loads into scalar registers.
// Plain form (vr_set_kernel_flavour(1), filter_plain_kernel): the same passes over the same regions, one lane per output reading its
// 2 r + 1 inputs straight from memory.  Same operations in the same order: the bits cannot differ.
// Write (filter_write_kernel): one lane per voxel of the box, one load of the last field (of the source with no pass), one 4-byte store
// into component dst_channel; the non-finite count and the least and greatest finite value (as keys that order the value bits with
// -0.0f below +0.0f) are folded across the wavefront behind the loop and reported with one atomic each.  Values move as 32-bit words:
// a NaN's payload survives a pure copy.
//
// Voxel indices are 64-bit throughout.  No kernel waits for another workgroup: the launch boundaries are the visibility points.
#pragma once
#include "vr_units.h"

namespace vr {

constexpr int kFilterMaxRadius = 32;                    // VR_FILTER_MAX_RADIUS
constexpr int kFilterMaxTaps = 2 * kFilterMaxRadius + 1;
constexpr int kFilterRun = 256;                         // outputs of a row per x tile ...
constexpr int kFilterRows = 8;                          // ... and the rows a workgroup takes at a time
constexpr int kFilterBatch = 8;                         // rows a wavefront of a y / z tile loads before it stores them
constexpr int kFilterT = 64;                            // outputs along the axis per y / z tile ...
constexpr int kFilterPerWave = kFilterT / 4;            // ... and per wavefront and lane

// f32 values over a region of the volume, x fastest: voxel (x, y, z) of the volume at p[index(x, y, z) * stride]
struct FilterView {
    float* p;
    int stride;        // floats between neighbours along x: 1 for a field, 4 for a component of the float4 voxels
    int lo[3], n[3];   // the region: first voxel and extent per axis
    __host__ __device__ size_t index(int x, int y, int z) const
    {
        return (((size_t)(z - lo[2]) * (size_t)n[1] + (size_t)(y - lo[1])) * (size_t)n[0] + (size_t)(x - lo[0])) * (size_t)stride;
    }
    __host__ __device__ unsigned long long voxels() const { return (unsigned long long)n[0] * (unsigned long long)n[1] * (unsigned long long)n[2]; }
};

// Kernel argument block of one pass: passed by value.
struct FilterPass {
    FilterView in, out;        // out: a field (stride 1) over this pass' region
    int r;                     // the radius
    int extent;                // voxels of the VOLUME along the pass' axis
    int border;                // VR_FILTER_CLAMP / VR_FILTER_CONSTANT
    float border_value;
    unsigned tx, ta;           // tiles along x; tiles along the axis (y / z passes)
    unsigned long long tiles;  // workgroup tiles of the default form
    float w[kFilterMaxTaps];   // w[0 .. 2 r]
};

// The device words of one vr_volume_filter: set by the host before the write, read behind it.
struct FilterWords {
    unsigned long long nonfinite;
    unsigned lo_key, hi_key;   // filter_key of the least / greatest finite stored value (start: ~0u, 0u)
};
// Kernel argument block of the write.
struct FilterWrite {
    FilterView in;             // the last pass' field, or the source
    unsigned* dst;             // the destination slot's x-fastest float4 voxels as words ...
    int dst_channel;           // ... and the component written
    int nx, ny;                // of the volume
    int lo[3], n[3];           // the box
    FilterWords* w;
};

// orders f32 bit patterns as their values, -0.0f below +0.0f (finite values only are compared)
__host__ __device__ __forceinline__ unsigned filter_key(unsigned bits) { return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u); }
__host__ __device__ __forceinline__ unsigned filter_unkey(unsigned key) { return (key & 0x80000000u) ? (key & 0x7fffffffu) : ~key; }

// the input of a pass along AXIS at voxel (x, y, z), whose coordinate on that axis may lie beyond the volume's faces
template <int AXIS>
__device__ __forceinline__ float filter_load(const FilterPass& P, int x, int y, int z)
{
    int& c = AXIS == 0 ? x : (AXIS == 1 ? y : z);
    if (c < 0 || c >= P.extent) {
        if (P.border != 0) return P.border_value;
        c = c < 0 ? 0 : P.extent - 1;
    }
    // (device memory, said outright: a global load, not a flat one whose wait the LDS traffic would share)
    return ((const __attribute__((address_space(1))) float*)P.in.p)[P.in.index(x, y, z)];
}

__global__ __launch_bounds__(256) void filter_x_kernel(const FilterPass P)
{
    __shared__ float tile[kFilterRows][kFilterRun + 2 * kFilterMaxRadius];
    const int r = P.r, tid = (int)threadIdx.x;
    const unsigned long long rows = (unsigned long long)P.out.n[1] * (unsigned long long)P.out.n[2];
    for (unsigned long long u = blockIdx.x; u < P.tiles; u += gridDim.x) {
        const unsigned long long g = u / P.tx;
        const int x0 = P.out.lo[0] + (int)(u - g * P.tx) * kFilterRun;
        const int left = P.out.lo[0] + P.out.n[0] - x0, run = left < kFilterRun ? left : kFilterRun;
        // rows g * kFilterRows .. of the region, y fastest; every lane loads its value of each row (and one of its halo), then stores them:
        // the loads of a tile are in flight together
        int y[kFilterRows], z[kFilterRows];
        float v[kFilterRows], h[kFilterRows];
#pragma unroll
        for (int q = 0; q < kFilterRows; ++q) {
            const unsigned long long row = g * kFilterRows + (unsigned)q;
            const unsigned long long sl = row / (unsigned)P.out.n[1];
            y[q] = row < rows ? P.out.lo[1] + (int)(row - sl * (unsigned)P.out.n[1]) : -1;
            z[q] = P.out.lo[2] + (int)sl;
            v[q] = h[q] = 0.0f;
            if (y[q] >= 0 && tid < run + 2 * r) v[q] = filter_load<0>(P, x0 - r + tid, y[q], z[q]);
            if (y[q] >= 0 && tid + 256 < run + 2 * r) h[q] = filter_load<0>(P, x0 - r + tid + 256, y[q], z[q]);
        }
#pragma unroll
        for (int q = 0; q < kFilterRows; ++q) {
            tile[q][tid] = v[q];
            if (tid < 2 * kFilterMaxRadius) tile[q][tid + 256] = h[q];
        }
        __syncthreads();
        if (tid < run) {  // (rows beyond the region are computed from zeros and never stored)
            float acc[kFilterRows];
            const float w0 = P.w[0];
#pragma unroll
            for (int q = 0; q < kFilterRows; ++q) acc[q] = w0 * tile[q][tid];
            for (int t = 1; t <= 2 * r; ++t) {
                const float wt = P.w[t];
#pragma unroll
                for (int q = 0; q < kFilterRows; ++q) acc[q] = fmaf(wt, tile[q][tid + t], acc[q]);
            }
#pragma unroll
            for (int q = 0; q < kFilterRows; ++q)
                if (y[q] >= 0) P.out.p[P.out.index(x0 + tid, y[q], z[q])] = acc[q];
        }
        __syncthreads();  // (the next tile overwrites this one)
    }
}

// AXIS = 1: along y, tiles over (x, y) for every z; AXIS = 2: along z, tiles over (x, z) for every y
template <int AXIS>
__global__ __launch_bounds__(256) void filter_line_kernel(const FilterPass P)
{
    extern __shared__ float rows[];  // (kFilterT + 2 r) rows of 64
    constexpr int OTHER = AXIS == 1 ? 2 : 1;
    const int r = P.r, lane = (int)(threadIdx.x & 63u);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    for (unsigned long long u = blockIdx.x; u < P.tiles; u += gridDim.x) {
        const unsigned long long v = u / P.tx, ib = v / P.ta;
        const int x = P.out.lo[0] + (int)(u - v * P.tx) * 64 + lane;
        const int a0 = P.out.lo[AXIS] + (int)(v - ib * P.ta) * kFilterT, b = P.out.lo[OTHER] + (int)ib;
        const int left = P.out.lo[AXIS] + P.out.n[AXIS] - a0, run = left < kFilterT ? left : kFilterT;
        const bool in_x = x < P.out.lo[0] + P.out.n[0];
        if (in_x)
            for (int k0 = wave; k0 < run + 2 * r; k0 += 4 * kFilterBatch) {  // a wavefront's rows, kFilterBatch loads in flight at a time
                float v[kFilterBatch];
#pragma unroll
                for (int q = 0; q < kFilterBatch; ++q) {
                    const int k = k0 + 4 * q;
                    v[q] = 0.0f;
                    if (k < run + 2 * r) v[q] = AXIS == 1 ? filter_load<1>(P, x, a0 - r + k, b) : filter_load<2>(P, x, b, a0 - r + k);
                }
#pragma unroll
                for (int q = 0; q < kFilterBatch; ++q)
                    if (k0 + 4 * q < run + 2 * r) rows[(k0 + 4 * q) * 64 + lane] = v[q];
            }
        __syncthreads();
        const int j0 = wave * kFilterPerWave;
        if (in_x && j0 < run) {  // (rows beyond the run are read as they lie and never stored: all within the tile)
            float acc[kFilterPerWave];
            const float w0 = P.w[0];
#pragma unroll
            for (int j = 0; j < kFilterPerWave; ++j) acc[j] = w0 * rows[(j0 + j) * 64 + lane];
            for (int t = 1; t <= 2 * r; ++t) {
                const float wt = P.w[t];
#pragma unroll
                for (int j = 0; j < kFilterPerWave; ++j) acc[j] = fmaf(wt, rows[(j0 + j + t) * 64 + lane], acc[j]);
            }
#pragma unroll
            for (int j = 0; j < kFilterPerWave; ++j)
                if (j0 + j < run) P.out.p[AXIS == 1 ? P.out.index(x, a0 + j0 + j, b) : P.out.index(x, b, a0 + j0 + j)] = acc[j];
        }
        __syncthreads();
    }
}

template <int AXIS>
__global__ __launch_bounds__(256) void filter_plain_kernel(const FilterPass P)
{
    const unsigned long long n = P.out.voxels(), step = (unsigned long long)gridDim.x * 256ull;
    const int r = P.r;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x; i < n; i += step) {
        const unsigned long long row = i / (unsigned)P.out.n[0], sl = row / (unsigned)P.out.n[1];
        int p[3] = {P.out.lo[0] + (int)(i - row * (unsigned)P.out.n[0]), P.out.lo[1] + (int)(row - sl * (unsigned)P.out.n[1]), P.out.lo[2] + (int)sl};
        const int c = p[AXIS];
        p[AXIS] = c - r;
        float acc = P.w[0] * filter_load<AXIS>(P, p[0], p[1], p[2]);
        for (int t = 1; t <= 2 * r; ++t) {
            p[AXIS] = c - r + t;
            acc = fmaf(P.w[t], filter_load<AXIS>(P, p[0], p[1], p[2]), acc);
        }
        P.out.p[i] = acc;
    }
}

__global__ __launch_bounds__(256) void filter_write_kernel(const FilterWrite W)
{
    const unsigned long long n = (unsigned long long)W.n[0] * (unsigned long long)W.n[1] * (unsigned long long)W.n[2];
    const unsigned long long step = (unsigned long long)gridDim.x * 256ull;
    const unsigned* const in = reinterpret_cast<const unsigned*>(W.in.p);
    unsigned long long nonfinite = 0ull;
    unsigned lo = ~0u, hi = 0u;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x; i < n; i += step) {
        const unsigned long long row = i / (unsigned)W.n[0], sl = row / (unsigned)W.n[1];
        const int x = W.lo[0] + (int)(i - row * (unsigned)W.n[0]), y = W.lo[1] + (int)(row - sl * (unsigned)W.n[1]), z = W.lo[2] + (int)sl;
        const unsigned bits = in[W.in.index(x, y, z)];
        W.dst[(((size_t)z * (size_t)W.ny + (size_t)y) * (size_t)W.nx + (size_t)x) * 4u + (size_t)W.dst_channel] = bits;
        if ((bits & 0x7f800000u) == 0x7f800000u) ++nonfinite;
        else {
            const unsigned k = filter_key(bits);
            lo = k < lo ? k : lo;
            hi = k > hi ? k : hi;
        }
    }
    nonfinite = wave_sum_u64(nonfinite);  // (behind the loop: every lane takes part in the folds)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned l = (unsigned)__shfl_down((int)lo, off, 64), h = (unsigned)__shfl_down((int)hi, off, 64);
        lo = l < lo ? l : lo;
        hi = h > hi ? h : hi;
    }
    if ((threadIdx.x & 63u) == 0u) {
        if (nonfinite != 0ull) atomicAdd(&W.w->nonfinite, nonfinite);
        if (lo <= hi) {  // (some finite value)
            atomicMin(&W.w->lo_key, lo);
            atomicMax(&W.w->hi_key, hi);
        }
    }
}

}  // namespace vr
