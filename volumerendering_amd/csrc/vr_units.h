// vr_units.h -- what the voxel tools share on the device.  Histograms (vr_hist.h) and region growing (vr_grow.h): a voxel box and the
// 4 x 4 x 4 BRICK UNITS of the volume's own brick grid that meet it, one step of the walk over them (the launch shape is described in
// vr_hist.h).  They and the bit-row tools (vr_bitrows.h, which has the walk over word rows; vr_morph.h, vr_dist.h, vr_raster.h): how a
// kernel reports (CountBox).  vr_device.h includes it: the structs are members of its argument blocks.
// (The two walks keep their own n_box / n_load / n_settled tail: a shared helper moved hist_kernel's row loop, masked histograms lost 1 %.)
#pragma once

namespace vr {

struct BoxUnits {  // (filled by box_units, vr_api_tools.h)
    int lo[3], hi[3];  // the voxel box, half open (hi <= n)
    int u0[3], un[3];  // the units that meet it: first unit and units per axis ...
    unsigned units;    // ... and their number (0 for an empty box)
};

// A voxel count and the half-open bounding box of the counted voxels: what a wavefront adds up and what it reports into.
struct CountBox {
    unsigned long long voxels;
    int lo[3], hi[3];
    static constexpr CountBox empty() { return {0ull, {0x7fffffff, 0x7fffffff, 0x7fffffff}, {0, 0, 0}}; }
};

// Unit u of a box's units (x fastest): its brick and the brick's first voxel.  uxy = un[0] * un[1], taken once in front of the loop.
struct BrickUnit { int bx, by, bz, x0, y0, z0; };
__device__ __forceinline__ BrickUnit brick_unit(const BoxUnits& B, unsigned u, unsigned uxy)
{
    const unsigned uz = u / uxy, ur = u - uz * uxy, uy = ur / (unsigned)B.un[0], ux = ur - uy * (unsigned)B.un[0];
    const int bx = B.u0[0] + (int)ux, by = B.u0[1] + (int)uy, bz = B.u0[2] + (int)uz;
    return {bx, by, bz, bx << 2, by << 2, bz << 2};
}
// The box holds all 64 voxels of the unit.  whole_unit<BoxUnits> copies the box: the six bounds are loaded first and the test compiles to
// selects (grow_classify_kernel); <const BoxUnits&> loads them as the && chain goes, with branches (hist_kernel): each kernel's old listing.
template <typename Box>
__device__ __forceinline__ bool whole_unit(Box B, const BrickUnit U)
{
    return U.x0 >= B.lo[0] && U.x0 + 4 <= B.hi[0] && U.y0 >= B.lo[1] && U.y0 + 4 <= B.hi[1] && U.z0 >= B.lo[2] && U.z0 + 4 <= B.hi[2];
}

__device__ __forceinline__ bool in_box(const BoxUnits& B, int x, int y, int z)
{
    return x >= B.lo[0] && x < B.hi[0] && y >= B.lo[1] && y < B.hi[1] && z >= B.lo[2] && z < B.hi[2];
}

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);  // (every lane takes part)
    return v;
}

// n voxels within [lo, hi) into *dst, which started as empty(): one add, three mins and three maxes (one lane calls it)
__device__ __forceinline__ void report_count_box(CountBox* dst, unsigned long long n, const int lo[3], const int hi[3])
{
    if (n == 0ull) return;
    atomicAdd(&dst->voxels, n);
    for (int a = 0; a < 3; ++a) {
        atomicMin(&dst->lo[a], lo[a]);
        atomicMax(&dst->hi[a], hi[a]);
    }
}

}  // namespace vr
