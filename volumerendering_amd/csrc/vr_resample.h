// vr_resample.h -- a volume slot resampled onto another grid (vr_volume_resample, include/vr.h): destination voxel (i, j, k) of the box
// lies at the source texture coordinate p = ((origin + i * di) + j * dj) + k * dk -- every operation rounded with separately rounded
// arithmetic, three nested fused multiply-adds mad(k, dk, mad(j, dj, mad(i, di, origin))) with fused arithmetic -- and stores, per
// selected component, textureSample(src, linear, p) (tex3_rgba: the clamp-to-edge texel pairs and seven lerps, in the arithmetic mode)
// or the voxel tex3_nearest addresses where p is inside the unit cube (slice_in_cube: NaN is outside), and outside[c] elsewhere.
// Components that are not selected and voxels outside the box are neither read nor written.  The uniforms, tables and viewport
// play no part: the kernel has a parameter struct of its own (ResampleParams, vr_device.h).  Included by vr_launch.h once per
// arithmetic mode.
//
// Work: persistent workgroups of four wavefronts walk the box in UNITS of 64 voxels along x of one row (unit u = 64-voxel piece
// u % ux of row u / ux, rows y fastest), one wavefront per unit, the lane being x: with all four components selected a wavefront
// stores 1 KiB of contiguous float4 into the x-fastest master copy.  Destination voxel indices are 64 bits (65535^3 is a legal grid);
// source voxel indices are the 32-bit slots of every gather here, in the layout in use.
//
// Forms (ResampleForm, vr_device.h).  kResamplePlain (vr_set_kernel_flavour(1)): every voxel is positioned and tested, every inside
// voxel fetches the corners of its float4 voxels.  kResampleDefault: the same behind a whole-wave test -- a wavefront none of whose
// lanes is inside stores `outside` without computing an address.  kResampleDensity, for a launch that writes component 3 alone:
// the corners come from the density plane behind a_base / a_shift (4 bytes per corner instead of 16, the same values), and a
// wavefront is SETTLED from the source's range records (brick_range_kernel, vr_prep.h) without a load where they allow it.
//
// Exact settling (LINEAR).  An inside lane's eight corners are the texel pairs i0 = clamp(t, 0, n - 1), i1 = clamp(t + 1, 0, n - 1) of
// t = (int)floor(mad(p, n, -0.5)) per axis (make_cell).  With b = clamp(t, 0, n - 1) >> 2 -- computed here from the same t, in
// integers -- both lie in [4 b, min(4 b + 4, n - 1)], the footprint of brick b's record (min, max) of .a; a record is (NaN, NaN)
// when a voxel of the footprint is NaN, infinite or above 2^125 in magnitude.  A lane's record SETTLES iff min == max as floats
// (false for a flagged record); then every corner compares equal to min, and, lerpf(a, b, t) being mad(b - a, t, a) with a finite
// weight t = x - floor(x) >= +0 (p is inside, so x is finite):
//   min != 0: equal non-zero floats are one bit pattern c, finite.  c - c = +0, (+0) * t = +0, +0 + c = c; fused, fma(+0, t, c) = c.
//     Each of the seven lerps returns c: the sample is c, bit for bit.
//   min == 0: the corners are +0 or -0 in any mix.  b - a is +0 (equal signs: x - x = +0 in round-to-nearest) or has b's sign, the
//     product with t >= +0 keeps that sign, and the sum with a is -0 only if both terms are -0: the product is -0 only for
//     (a, b) = (+0, -0), whose a is +0.  So every first-level lerp returns +0, fused or not (the product is exact either way), and
//     the later levels lerp +0 with +0: the sample is +0.0f, also over a brick of -0 alone.
// A wavefront whose inside lanes ALL settle stores those values without computing an address and counts none of its voxels as
// loaded; one lane that does not settle and the whole wavefront loads (the loads return the same bits).  NEAREST returns a voxel
// as it is, and a record of zero does not say which zero: the filter does not settle (nor would the base cell's brick be the right
// one to ask without the argument of vr_slice.h).
//
// Result words (ResampleWords): every wavefront adds its inside voxels, their bounding box and its loaded voxels once, behind its
// last unit.
#pragma once

namespace VR_KNS {

__device__ __forceinline__ f3 resample_position(const ResampleParams& R, int i, int j, int k)
{
    const float fi = (float)i, fj = (float)j, fk = (float)k;
    return mk3(mad(fk, R.dk[0], mad(fj, R.dj[0], mad(fi, R.di[0], R.origin[0]))), mad(fk, R.dk[1], mad(fj, R.dj[1], mad(fi, R.di[1], R.origin[1]))),
               mad(fk, R.dk[2], mad(fj, R.dj[2], mad(fi, R.di[2], R.origin[2]))));
}

// record of the brick of p's base cell, from make_cell's own floored coordinate
__device__ __forceinline__ float2 resample_record(const ResampleParams& R, f3 p)
{
    const DevVolume& v = R.src;
    const int bx = clampi((int)floorf(mad(p.x, (float)v.nx, -0.5f)), 0, v.nx - 1) >> kBrickShift;
    const int by = clampi((int)floorf(mad(p.y, (float)v.ny, -0.5f)), 0, v.ny - 1) >> kBrickShift;
    const int bz = clampi((int)floorf(mad(p.z, (float)v.nz, -0.5f)), 0, v.nz - 1) >> kBrickShift;
    return R.bricks[((size_t)bz * (size_t)R.bny + (size_t)by) * (size_t)R.bnx + (size_t)bx];
}

template <bool NEAREST, bool OFF32, int FORM>
__global__ __launch_bounds__(256) void resample_kernel(const ResampleParams R)
{
    const int lane = (int)(threadIdx.x & 63u);
    const unsigned wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const unsigned long long first = (unsigned long long)blockIdx.x * 4ull + wave, stride = (unsigned long long)gridDim.x * 4ull;
    const unsigned rows_y = (unsigned)(R.hi[1] - R.lo[1]);
    // unit u = piece xu of row `row`; the walk advances both without a division per unit
    const unsigned step_rows = (unsigned)(stride / R.ux), step_xu = (unsigned)(stride % R.ux);
    unsigned long long row = first / R.ux;
    unsigned xu = (unsigned)(first % R.ux);
    unsigned long long n_in = 0, n_load = 0;  // (wave-uniform)
    int min_x = 0x7fffffff, max_x = 0, min_y = 0x7fffffff, max_y = 0, min_z = 0x7fffffff, max_z = 0;  // x per lane, y / z wave-uniform
    for (unsigned long long u = first; u < R.units; u += stride) {
        const unsigned zr = (unsigned)row / rows_y, yr = (unsigned)row - zr * rows_y;  // (rows of a box: below 2^32)
        const int x = R.lo[0] + (int)(xu << 6) + lane, y = R.lo[1] + (int)yr, z = R.lo[2] + (int)zr;
        const bool active = x < R.hi[0];
        const f3 p = resample_position(R, x, y, z);
        const bool in = active && slice_in_cube(p);
        const unsigned long long in_mask = vr_ballot(in);
        float4 val = make_float4(R.outside[0], R.outside[1], R.outside[2], R.outside[3]);
        if (FORM == kResamplePlain || in_mask != 0ull) {
            bool load = in;
            if constexpr (FORM == kResampleDensity && !NEAREST) {
                if (R.bricks) {  // (wave-uniform)
                    float2 rec = make_float2(0.0f, 1.0f);
                    if (in) rec = resample_record(R, p);
                    const bool settles = rec.x == rec.y;
                    if (vr_ballot(in && !settles) == 0ull) {
                        load = false;
                        if (in) val.w = rec.x == 0.0f ? 0.0f : rec.x;
                    }
                }
            }
            if (load) {
                if constexpr (FORM == kResampleDensity) {
                    if constexpr (NEAREST) val.w = load_a<OFF32>(R.src, slice_nearest_slot(R.src, p));
                    else val.w = tex3_a<OFF32>(R.src, p);
                } else {
                    if constexpr (NEAREST) val = tex3_nearest<OFF32>(R.src, p);
                    else val = tex3_rgba<OFF32>(R.src, p);
                }
            }
            n_load += (unsigned long long)__popcll(vr_ballot(load));
        }
        if (active) {
            float4* d = R.dst + (((size_t)z * (size_t)R.n[1] + (size_t)y) * (size_t)R.n[0] + (size_t)x);
            if constexpr (FORM == kResampleDensity) {
                reinterpret_cast<float*>(d)[3] = val.w;
            } else if (R.channels == 15u) {
                *d = val;
            } else {  // (wave-uniform: the selected components alone)
                float* f = reinterpret_cast<float*>(d);
                if (R.channels & 1u) f[0] = val.x;
                if (R.channels & 2u) f[1] = val.y;
                if (R.channels & 4u) f[2] = val.z;
                if (R.channels & 8u) f[3] = val.w;
            }
        }
        if (in_mask != 0ull) {
            n_in += (unsigned long long)__popcll(in_mask);
            min_y = min(min_y, y), max_y = max(max_y, y + 1);
            min_z = min(min_z, z), max_z = max(max_z, z + 1);
            if (in) min_x = min(min_x, x), max_x = max(max_x, x + 1);
        }
        row += step_rows;
        xu += step_xu;
        if (xu >= R.ux) xu -= R.ux, ++row;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {  // (every lane takes part)
        min_x = min(min_x, __shfl_down(min_x, off, 64));
        max_x = max(max_x, __shfl_down(max_x, off, 64));
    }
    if (lane == 0) {
        const int lo[3] = {min_x, min_y, min_z}, hi[3] = {max_x, max_y, max_z};
        report_count_box(&R.w->inside, n_in, lo, hi);
        if (n_load != 0ull) atomicAdd(&R.w->loaded, n_load);
    }
}

}  // namespace VR_KNS
