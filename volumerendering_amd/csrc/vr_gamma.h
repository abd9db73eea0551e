// vr_gamma.h -- the gamma index of two dose channels on the device (vr_volume_gamma, include/vr.h): for every voxel p of a box the least,
// over the admitted candidate positions around p, of g2 = fmaf(d, d, c) with d = (e - r) * invT the dose difference in tolerances and c
// the squared distance in distances-to-agreement; the square root goes into one component of a volume slot.  The arithmetic is the
// header's, every step named there: one rounded subtraction and one explicit fmaf per interpolation, one subtraction, one product and one
// fmaf per candidate.  vr_set_arithmetic plays no part (the unit is compiled with -ffp-contract=off, and an fmaf is an fmaf under either
// flag), which is why these kernels exist once, included by vr_api.hip alone.
//
// The TABLE (GammaEntry, built and uploaded by the host once per call) holds the K admitted offsets in ascending D2n, ties by (k, j, i):
// per entry the base-voxel step m (floor(o / sub) per axis), the sub-step f and c = (float)D2n * kc.  Entry 0 is the offset (0, 0, 0),
// which always exists; behind entry K - 1 stands a copy of it, so that the default form may load one entry ahead.  Every lane of a
// wavefront walks the table at the same index: an entry is a scalar load.
//
// Two facts carry both forms (include/vr.h says why they hold):
//   ORDER  g2 is +0 or positive, never -0, and a NaN g2 is ignored: the least g2 is one bit pattern in whatever order candidates come.
//   CUT    g2 >= c always (rounding is monotone, d * d >= 0).  A candidate whose c is not below a voxel's running minimum cannot lower
//          it; c ascends along the table, so a voxel is finished at the first such entry.
//
// Default form (gamma_tile_kernel): a workgroup of 256 lanes takes a tile of kGammaTX x kGammaTY x kGammaTZ = 32 x 8 x 4 outputs of the
// box (x, y, z), four per lane (same x and y, the four z), and stages E for the tile grown by the halo h_a = reach / spacing[a] (+ 1
// with sub > 1: the upper corner of an interpolation, and the base voxel of a negative sub-step) once into dynamic LDS: (32 + 2 hx) *
// (8 + 2 hy) * (4 + 2 hz) floats -- 27.5 KiB for the clinical 3 mm / 6 mm reach at 1 x 1 x 3 mm and sub 1 (h = 6, 6, 2: five workgroups
// per CU of 160 KiB), 111.7 KiB at the worst (h = 9, 9, 9: one).  No radius the descriptor admits is too large for the tile: there is no
// fall-back per axis.  A wavefront stages a row of the grown tile, one word per lane, kGammaBatch = 4 rows at a time: four
// unconditional loads from clamped addresses in flight per lane, then the stores.  A position outside the VOLUME is staged as NaN: e is then NaN (a lerp with a NaN corner is NaN; an axis with
// f_a == 0 never reads its upper corner), g2 is NaN, and a NaN g2 is ignored -- exactly "not a candidate", with no bounds test in the
// loop.  Lanes run along x, 32 per row: a ds_read_b32 serves two rows of 32 neighbouring words per instruction, free of bank conflicts
// whatever the row stride.  A lane asks for entry k while c_k is below one of its four running minima (kept as bits: gamma_min says why
// an unsigned minimum is the header's); the wavefront leaves the loop at the first entry no lane asks for.  A lane that no longer asks
// still computes in step with the others: by CUT its minima cannot change.  Lanes outside the box and skipped voxels start at a minimum
// of +0 and never ask.
// Plain form (vr_set_kernel_flavour(1), gamma_plain_kernel): one lane per output voxel, every admitted candidate, existence tested per
// axis as the header states it, every corner read from memory, no cut: the on-device cross-check and the baseline.
// Both write a FIELD: two words per voxel of the box, x fastest -- the bits to store and the flags kGammaEvaluated | kGammaPassed.
// Write (gamma_write_kernel): one lane per voxel of the box: one 8-byte load of the field, one 4-byte store into component dst_channel;
// the counts and the greatest finite stored value of evaluated voxels (stored values are +0 or positive: their bits order as they do)
// are folded across the wavefront behind the loop and reported with one atomic each.  The search kernels have read R, E and the ROI
// before the write is launched: the destination may be any of them.
//
// Voxel indices are 64-bit throughout.  No kernel waits for another workgroup: the launch boundaries are the visibility points.
#pragma once
#include "vr_units.h"  // wave_sum_u64

namespace vr {

constexpr int kGammaMaxSub = 4, kGammaMaxRadius = 8;    // VR_GAMMA_MAX_SUB, VR_GAMMA_MAX_RADIUS
constexpr int kGammaTX = 32, kGammaTY = 8, kGammaTZ = 4;  // outputs of a tile along x, y, z: kGammaTX * kGammaTY lanes, kGammaTZ outputs each
constexpr int kGammaMaxHalo = kGammaMaxRadius + 1;
constexpr int kGammaBatch = 4;                          // rows of the grown tile a wavefront loads before it stores them
static_assert(kGammaTX + 2 * kGammaMaxHalo <= 64, "a wavefront stages a row of the grown tile, one word per lane");
constexpr unsigned kGammaMaxLds = (kGammaTX + 2 * kGammaMaxHalo) * (kGammaTY + 2 * kGammaMaxHalo) * (kGammaTZ + 2 * kGammaMaxHalo) * 4u;
constexpr unsigned kGammaEvaluated = 1u, kGammaPassed = 2u;
constexpr unsigned kGammaNan = 0x7fc00000u;

// An admitted offset: bits 0 .. 4 m_x + 16, 5 .. 9 m_y + 16, 10 .. 14 m_z + 16, 15 .. 16 f_x, 17 .. 18 f_y, 19 .. 20 f_z; c.
struct GammaEntry {
    unsigned packed;
    float c;
};
__host__ __device__ __forceinline__ unsigned gamma_pack(const int m[3], const int f[3])
{
    return (unsigned)(m[0] + 16) | (unsigned)(m[1] + 16) << 5 | (unsigned)(m[2] + 16) << 10 | (unsigned)f[0] << 15 | (unsigned)f[1] << 17 | (unsigned)f[2] << 19;
}

// Kernel argument block of a search: passed by value.
struct GammaArgs {
    const float* ref;          // the reference slot's x-fastest float4 voxels as floats, ref_channel added
    const float* eval;         // the evaluated slot's, eval_channel added
    const float* roi;          // the ROI slot's, roi_contour added; nullptr: none
    int n[3];                  // of the volume
    int lo[3], bn[3];          // the box: first voxel and extent per axis
    int h[3];                  // the halo of a tile per axis (default form)
    int sub;
    float t[kGammaMaxSub];     // t[f] = (float)f / (float)sub
    int mode;                  // VR_GAMMA_GLOBAL / VR_GAMMA_LOCAL
    float tol, cutoff;
    unsigned skip_bits;
    const GammaEntry* table;
    unsigned K;
    uint2* out;                // the field: two words per voxel of the box, x fastest
    unsigned tx, ty;           // tiles along x and y (default form)
    unsigned long long tiles;  // workgroup tiles of the default form
};

// The device words of one vr_volume_gamma: set by the host before the write, read behind it.
struct GammaWords {
    unsigned long long evaluated, passed, nonfinite;
    unsigned hi_bits, pad;     // the bits of the greatest finite stored value of an evaluated voxel (start: 0)
};
// Kernel argument block of the write.
struct GammaWrite {
    const uint2* field;        // two words per voxel of the box
    unsigned* dst;             // the destination's voxels as words, dst_channel added
    int nx, ny;                // of the volume
    int lo[3], n[3];           // the box
    GammaWords* w;
};

__device__ __forceinline__ size_t gamma_at(const GammaArgs& A, int x, int y, int z)
{
    return (((size_t)z * (size_t)A.n[1] + (size_t)y) * (size_t)A.n[0] + (size_t)x) * 4u;
}
// (device memory, said outright: a global load, not a flat one whose wait the LDS traffic would share)
__device__ __forceinline__ float gamma_global(const float* p, size_t i) { return ((const __attribute__((address_space(1))) float*)p)[i]; }

// invT of a voxel whose reference dose is r and whose ROI component is m (anything but 0 without an ROI); false: the voxel is skipped
__device__ __forceinline__ bool gamma_evaluated(const GammaArgs& A, float r, float m, float& inv_t)
{
    const float T = A.mode != 0 ? A.tol * r : A.tol;
    inv_t = 1.0f / T;
    // (a NaN r or T fails its comparison; in the ROI: NaN is in, -0.0f is out)
    return r >= A.cutoff && T > 0.0f && T <= 3.402823466e+38f && m != 0.0f;
}
// r and invT of voxel (x, y, z) of the volume; false: the voxel is skipped
__device__ __forceinline__ bool gamma_tolerance(const GammaArgs& A, int x, int y, int z, float& r, float& inv_t)
{
    const size_t at = gamma_at(A, x, y, z);
    r = gamma_global(A.ref, at);
    return gamma_evaluated(A, r, A.roi ? gamma_global(A.roi, at) : 1.0f, inv_t);
}
__device__ __forceinline__ int gamma_clamp(int v, int n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }

// e at a candidate: at(dx, dy, dz) is E at the base voxel's corner (dx, dy, dz); along x, then y, then z; an axis with f == 0 takes its
// lower value as it is and does not read the upper one
template <typename At>
__device__ __forceinline__ float gamma_interp(At at, unsigned fx, unsigned fy, unsigned fz, float tx, float ty, float tz)
{
    auto along_x = [&](int dy, int dz) {
        const float u = at(0, dy, dz);
        return fx != 0u ? fmaf(tx, at(1, dy, dz) - u, u) : u;
    };
    auto along_y = [&](int dz) {
        const float u = along_x(0, dz);
        return fy != 0u ? fmaf(ty, along_x(1, dz) - u, u) : u;
    };
    const float u = along_y(0);
    return fz != 0u ? fmaf(tz, along_y(1) - u, u) : u;
}

// The running minimum travels as BITS, started at kGammaNone.  g2 is +0, positive or NaN: as unsigned integers the bits of the values
// that are no NaN order as the values do, and every NaN, of either sign, lies above +inf's bits.  One v_min_u32 therefore ignores a NaN
// g2, lets the start value and a NaN minimum give way, and never touches a payload.
constexpr unsigned kGammaNone = 0xffffffffu, kGammaInf = 0x7f800000u;
__device__ __forceinline__ unsigned gamma_min(unsigned best, float g2)
{
    const unsigned b = __float_as_uint(g2);
    return b < best ? b : best;
}
// entry k of the table: constant for the whole launch and the same k in every lane -- a scalar load
__device__ __forceinline__ GammaEntry gamma_entry(const GammaArgs& A, unsigned k)
{
    const unsigned long long w = ((const __attribute__((address_space(4))) unsigned long long*)A.table)[k];  // (packed low, c high)
    GammaEntry e;
    e.packed = (unsigned)w;
    e.c = __uint_as_float((unsigned)(w >> 32));
    return e;
}

// the field's words of a voxel: best = the bits of G2 (above +inf's: every g2 was NaN)
__device__ __forceinline__ uint2 gamma_words(const GammaArgs& A, bool evaluated, unsigned best)
{
    if (!evaluated) return make_uint2(A.skip_bits, 0u);
    if (best > kGammaInf) return make_uint2(kGammaNan, kGammaEvaluated);
    return make_uint2(__float_as_uint(sqrtf(__uint_as_float(best))), kGammaEvaluated | (best <= 0x3f800000u ? kGammaPassed : 0u));
}

template <bool INTERP>
__global__ __launch_bounds__(256) void gamma_tile_kernel(const GammaArgs A)
{
    extern __shared__ float gamma_tile[];
    const int tid = (int)threadIdx.x, lx = tid & (kGammaTX - 1), ly = tid >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int hx = A.h[0], hy = A.h[1], hz = A.h[2];
    const int ex = kGammaTX + 2 * hx, ey = kGammaTY + 2 * hy, ez = kGammaTZ + 2 * hz, slab = ex * ey;
    const float nan = __uint_as_float(kGammaNan);
    for (unsigned long long u = blockIdx.x; u < A.tiles; u += gridDim.x) {
        const unsigned long long g = u / A.tx, h = g / A.ty;
        const int x0 = (int)(u - g * A.tx) * kGammaTX, y0 = (int)(g - h * A.ty) * kGammaTY, z0 = (int)h * kGammaTZ;  // within the box
        // Staging, row by row: a wavefront takes a row of the grown tile (ex <= 64 words: lane = x) and kGammaBatch rows (y) at a time.
        // Every load is unconditional, from the address clamped into the volume, so the kGammaBatch loads of a lane are in flight
        // together; what lies outside the volume becomes NaN by a select behind them, and only then come the stores.  y and z of a row
        // are wave-uniform: no division per word.
        const int sx = A.lo[0] + x0 - hx + lane, cx = gamma_clamp(sx, A.n[0]);
        const bool x_in = (unsigned)sx < (unsigned)A.n[0];
        for (int iz = 0; iz < ez; ++iz) {
            const int sz = A.lo[2] + z0 - hz + iz, cz = gamma_clamp(sz, A.n[2]);
            const bool xz_in = x_in && (unsigned)sz < (unsigned)A.n[2];
            for (int iy0 = wave * kGammaBatch; iy0 < ey; iy0 += 4 * kGammaBatch) {
                float v[kGammaBatch];
#pragma unroll
                for (int b = 0; b < kGammaBatch; ++b) {
                    const int sy = A.lo[1] + y0 - hy + iy0 + b;
                    const float e = gamma_global(A.eval, gamma_at(A, cx, gamma_clamp(sy, A.n[1]), cz));
                    v[b] = xz_in && (unsigned)sy < (unsigned)A.n[1] ? e : nan;
                }
#pragma unroll
                for (int b = 0; b < kGammaBatch; ++b)
                    if (lane < ex && iy0 + b < ey) gamma_tile[(iz * ey + iy0 + b) * ex + lane] = v[b];
            }
        }
        __syncthreads();
        const int x = x0 + lx, y = y0 + ly;
        const bool in_xy = x < A.bn[0] && y < A.bn[1];
        float r[kGammaTZ], inv_t[kGammaTZ], roi[kGammaTZ];
        unsigned best[kGammaTZ];
        bool evaluated[kGammaTZ];
        // R and the ROI of the lane's four outputs, loaded together from addresses clamped into the volume (a lane beyond the box's end)
        const int vx = gamma_clamp(A.lo[0] + x, A.n[0]), vy = gamma_clamp(A.lo[1] + y, A.n[1]);
        size_t at[kGammaTZ];
#pragma unroll
        for (int q = 0; q < kGammaTZ; ++q) {
            at[q] = gamma_at(A, vx, vy, gamma_clamp(A.lo[2] + z0 + q, A.n[2]));
            r[q] = gamma_global(A.ref, at[q]);
            roi[q] = 1.0f;
        }
        if (A.roi) {  // (one branch around the four loads, not one around each)
#pragma unroll
            for (int q = 0; q < kGammaTZ; ++q) roi[q] = gamma_global(A.roi, at[q]);
        }
#pragma unroll
        for (int q = 0; q < kGammaTZ; ++q) {
            evaluated[q] = gamma_evaluated(A, r[q], roi[q], inv_t[q]) && in_xy && z0 + q < A.bn[2];
            best[q] = evaluated[q] ? kGammaNone : 0u;  // (+0: no c is below it, and no g2 lowers it)
        }
        const float* const p = gamma_tile + (hz * ey + hy + ly) * ex + hx + lx;  // the lane's first output; output q is q slabs on
        GammaEntry next = gamma_entry(A, 0u);
        for (unsigned k = 0; k < A.K; ++k) {
            const GammaEntry en = next;
            next = gamma_entry(A, k + 1u);  // (issued beside this trip's LDS reads and waited for with them, not at the head of the next trip
                                            // on its own; the table ends with a copy of its last entry for this)
            const float c = en.c;
            bool asking = false;
#pragma unroll
            for (int q = 0; q < kGammaTZ; ++q) asking = asking || __float_as_uint(c) < best[q];  // (c is +0 or positive: its bits order too)
            if (!__any(asking)) break;
            const int mx = (int)(en.packed & 31u) - 16, my = (int)((en.packed >> 5) & 31u) - 16, mz = (int)((en.packed >> 10) & 31u) - 16;
            const float* const b = p + (mz * ey + my) * ex + mx;
            const unsigned fx = (en.packed >> 15) & 3u, fy = (en.packed >> 17) & 3u, fz = (en.packed >> 19) & 3u;
#pragma unroll
            for (int q = 0; q < kGammaTZ; ++q) {
                const float* const bq = b + q * slab;
                const float e = INTERP ? gamma_interp([&](int dx, int dy, int dz) { return bq[(dz * ey + dy) * ex + dx]; }, fx, fy, fz, A.t[fx], A.t[fy], A.t[fz])
                                       : bq[0];
                const float d = (e - r[q]) * inv_t[q];
                best[q] = gamma_min(best[q], fmaf(d, d, c));
            }
        }
#pragma unroll
        for (int q = 0; q < kGammaTZ; ++q) {
            const int z = z0 + q;
            if (!in_xy || z >= A.bn[2]) continue;
            A.out[((size_t)z * (size_t)A.bn[1] + (size_t)y) * (size_t)A.bn[0] + (size_t)x] = gamma_words(A, evaluated[q], best[q]);
        }
        __syncthreads();  // (the next tile overwrites this one)
    }
}

__global__ __launch_bounds__(256) void gamma_plain_kernel(const GammaArgs A)
{
    const unsigned long long n = (unsigned long long)A.bn[0] * (unsigned long long)A.bn[1] * (unsigned long long)A.bn[2];
    const unsigned long long step = (unsigned long long)gridDim.x * 256ull;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x; i < n; i += step) {
        const unsigned long long row = i / (unsigned)A.bn[0], sl = row / (unsigned)A.bn[1];
        const int x = A.lo[0] + (int)(i - row * (unsigned)A.bn[0]), y = A.lo[1] + (int)(row - sl * (unsigned)A.bn[1]), z = A.lo[2] + (int)sl;
        float r, inv_t;
        unsigned best = kGammaNone;
        const bool evaluated = gamma_tolerance(A, x, y, z, r, inv_t);
        for (unsigned k = 0; evaluated && k < A.K; ++k) {
            const GammaEntry en = gamma_entry(A, k);
            const int bx = x + (int)(en.packed & 31u) - 16, by = y + (int)((en.packed >> 5) & 31u) - 16, bz = z + (int)((en.packed >> 10) & 31u) - 16;
            const unsigned fx = (en.packed >> 15) & 3u, fy = (en.packed >> 17) & 3u, fz = (en.packed >> 19) & 3u;
            const bool exists = bx >= 0 && bx + (fx != 0u ? 1 : 0) <= A.n[0] - 1 && by >= 0 && by + (fy != 0u ? 1 : 0) <= A.n[1] - 1 &&
                                bz >= 0 && bz + (fz != 0u ? 1 : 0) <= A.n[2] - 1;
            if (!exists) continue;
            const float e = gamma_interp([&](int dx, int dy, int dz) { return gamma_global(A.eval, gamma_at(A, bx + dx, by + dy, bz + dz)); },
                                         fx, fy, fz, A.t[fx], A.t[fy], A.t[fz]);
            const float d = (e - r) * inv_t;
            best = gamma_min(best, fmaf(d, d, en.c));
        }
        A.out[i] = gamma_words(A, evaluated, best);
    }
}

__global__ __launch_bounds__(256) void gamma_write_kernel(const GammaWrite W)
{
    const unsigned long long n = (unsigned long long)W.n[0] * (unsigned long long)W.n[1] * (unsigned long long)W.n[2];
    const unsigned long long step = (unsigned long long)gridDim.x * 256ull;
    unsigned long long evaluated = 0ull, passed = 0ull, nonfinite = 0ull;
    unsigned hi = 0u;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x; i < n; i += step) {
        const unsigned long long row = i / (unsigned)W.n[0], sl = row / (unsigned)W.n[1];
        const int x = W.lo[0] + (int)(i - row * (unsigned)W.n[0]), y = W.lo[1] + (int)(row - sl * (unsigned)W.n[1]), z = W.lo[2] + (int)sl;
        const uint2 f = W.field[i];
        W.dst[(((size_t)z * (size_t)W.ny + (size_t)y) * (size_t)W.nx + (size_t)x) * 4u] = f.x;
        if ((f.y & kGammaEvaluated) == 0u) continue;
        ++evaluated;
        if ((f.y & kGammaPassed) != 0u) ++passed;
        if ((f.x & 0x7f800000u) == 0x7f800000u) ++nonfinite;
        else hi = f.x > hi ? f.x : hi;
    }
    evaluated = wave_sum_u64(evaluated);  // (behind the loop: every lane takes part in the folds)
    passed = wave_sum_u64(passed);
    nonfinite = wave_sum_u64(nonfinite);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned h = (unsigned)__shfl_down((int)hi, off, 64);
        hi = h > hi ? h : hi;
    }
    if ((threadIdx.x & 63u) == 0u) {
        if (evaluated != 0ull) atomicAdd(&W.w->evaluated, evaluated);
        if (passed != 0ull) atomicAdd(&W.w->passed, passed);
        if (nonfinite != 0ull) atomicAdd(&W.w->nonfinite, nonfinite);
        if (hi != 0u) atomicMax(&W.w->hi_bits, hi);
    }
}

}  // namespace vr
