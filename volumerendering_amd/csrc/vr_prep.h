// vr_prep.h -- what happens to a volume between its upload and the first march: the data-preparation passes, the bricked copy, the
// density plane and the check of a derived gradient, and the brick records (maximum and range per empty-space brick) that the
// skipping marches, the projections and the voxel tools read.  Streaming kernels with no per-sample arithmetic: they exist once, in
// namespace vr, and only the C ABI's translation unit (vr_api.hip) includes them.
#pragma once
#include "vr_device.h"
#include "vr_shared.h"  // vr_ballot

namespace vr {

// ------------------------------------------------------------------------------------------------ data preparation
//  the reference's single-threaded CPU passes over the voxels, as HBM-bound streaming kernels.

template <typename T>
__global__ void broadcast_raw_kernel(const T* __restrict__ raw, float4* __restrict__ vol, size_t n)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) {
        float v = (float)raw[i];
        vol[i] = make_float4(v, v, v, v);
    }
}

// out[0] = max over voxels of component `comp` (as f32 bits; values are >= 0 in every use: raw data, magnitudes)
__global__ void max_component_kernel(const float4* __restrict__ vol, size_t n, int comp, unsigned* __restrict__ out)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    float m = 0.0f;
    for (; i < n; i += stride) {
        float4 v = vol[i];
        float c = comp == 0 ? v.x : (comp == 1 ? v.y : (comp == 2 ? v.z : v.w));
        if (m < c) m = c;  // std::max_element semantics of GetMaxNumber: NaNs never win
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_down(m, off, 64));
    if ((threadIdx.x & 63) == 0) atomicMax(out, __float_as_uint(m));  // non-negative floats order like their bits
}

__global__ void normalize_kernel(float4* __restrict__ vol, size_t n, int value)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const float d = (float)value;
    for (; i < n; i += stride) {
        float4 v = vol[i];
        v.w = v.w / d;
        vol[i] = v;
    }
}

// One thread per voxel, x fastest (coalesced); the density is read from the untouched .w lanes, so the pass can
// run in place.  max_mag (f32 bits) accumulates the largest |gradient| when requested.
__global__ void gradient_kernel(float4* __restrict__ vol, int nx, int ny, int nz, int want_max, unsigned* __restrict__ max_mag)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y, z = blockIdx.z;
    float mag = 0.0f;
    if (x < nx) {
        const size_t row = ((size_t)z * ny + y) * nx;
        const size_t c = row + x;
        const size_t sy = (size_t)nx, sz = (size_t)nx * ny;
        float mx = x > 0 ? vol[c - 1].w : 0.0f, px = x + 1 < nx ? vol[c + 1].w : 0.0f;
        float my = y > 0 ? vol[c - sy].w : 0.0f, py = y + 1 < ny ? vol[c + sy].w : 0.0f;
        float mz = z > 0 ? vol[c - sz].w : 0.0f, pz = z + 1 < nz ? vol[c + sz].w : 0.0f;
        float tx = (-(px - mx)) * 0.5f, ty = (-(py - my)) * 0.5f, tz = (-(pz - mz)) * 0.5f;
        if (want_max) mag = sqrtf((tx * tx + ty * ty) + tz * tz);
        float* o = reinterpret_cast<float*>(vol + c);
        o[0] = tx;
        o[1] = ty;
        o[2] = tz;
    }
    if (want_max) {
        if (!(mag > 0.0f)) mag = 0.0f;  // `if (mag > maxGradMag)`: NaN never wins
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) mag = fmaxf(mag, __shfl_down(mag, off, 64));
        if ((threadIdx.x & 63) == 0 && mag > 0.0f) atomicMax(max_mag, __float_as_uint(mag));
    }
}

__global__ void scale_gradient_kernel(float4* __restrict__ vol, size_t n, const unsigned* __restrict__ max_mag)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const float d = __uint_as_float(*max_mag);
    for (; i < n; i += stride) {
        float4 v = vol[i];
        v.x = v.x / d;
        v.y = v.y / d;
        v.z = v.z / d;
        vol[i] = v;
    }
}

// ---- bricked copy of a volume (DevVolume::bricked; rebuilt with the brick records after every upload or in-place change) -----
// One thread per slot of the bricked arrays: slot s = brick * 64 + (lz * 16 + ly * 4 + lx) for the default 4 x 4 x 4 bricks;
// voxels beyond the volume's faces (the last brick of an axis whose size is not a multiple of the brick edge) are zero and
// never addressed.
__global__ void rebrick_kernel(const float4* __restrict__ lin, float4* __restrict__ bvol, float* __restrict__ bdens, int nx, int ny,
                               int nz, unsigned nbx, unsigned nby, size_t n_slots)
{
    size_t s = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (; s < n_slots; s += stride) {
        const unsigned l = (unsigned)(s & (kVbN - 1u));
        const size_t b = s >> (3u * kVbS);
        const unsigned bx = (unsigned)(b % nbx), by = (unsigned)((b / nbx) % nby), bz = (unsigned)(b / ((size_t)nbx * nby));
        const int x = (int)((bx << kVbS) + (l & kVbM)), y = (int)((by << kVbS) + ((l >> kVbS) & kVbM)), z = (int)((bz << kVbS) + (l >> (2u * kVbS)));
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (x < nx && y < ny && z < nz) v = lin[((size_t)z * ny + y) * nx + x];
        bvol[s] = v;
        bdens[s] = v.w;
    }
}

// ---- density plane / derived-gradient check (run with the brick records after every upload or in-place change) -------
__global__ void extract_density_kernel(const float4* __restrict__ vol, float* __restrict__ dens, size_t n)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) dens[i] = vol[i].w;
}
// *mismatch != 0 afterwards unless EVERY voxel's .rgb has exactly the bits PreComputeGradient(false) computes from the
// .a plane ((-(p - m)) * 0.5 per axis, neighbours outside the grid = 0; NaNs never match).
__device__ __forceinline__ float grad_cd(float p, float m) { return (-(p - m)) * 0.5f; }
__global__ void verify_gradient_kernel(const float4* __restrict__ vol, const float* __restrict__ dens, int nx, int ny, int nz,
                                       unsigned* __restrict__ mismatch)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y, z = blockIdx.z;
    bool bad = false;
    if (x < nx) {
        const size_t c = ((size_t)z * ny + y) * nx + x;
        const size_t sy = (size_t)nx, sz = (size_t)nx * ny;
        const float mx = x > 0 ? dens[c - 1] : 0.0f, px = x + 1 < nx ? dens[c + 1] : 0.0f;
        const float my = y > 0 ? dens[c - sy] : 0.0f, py = y + 1 < ny ? dens[c + sy] : 0.0f;
        const float mz = z > 0 ? dens[c - sz] : 0.0f, pz = z + 1 < nz ? dens[c + sz] : 0.0f;
        const float4 v = vol[c];
        bad = __float_as_uint(v.x) != __float_as_uint(grad_cd(px, mx)) || __float_as_uint(v.y) != __float_as_uint(grad_cd(py, my)) ||
              __float_as_uint(v.z) != __float_as_uint(grad_cd(pz, mz)) || v.x != v.x || v.y != v.y || v.z != v.z;
    }
    if (vr_ballot(bad) != 0 && (threadIdx.x & 63) == 0) atomicOr(mismatch, 1u);
}

// ---- brick records (rebuilt with the bricked copy) ----------------------------------------------------------------
// One wavefront per brick of c = kBrickCells cells: maximum of .a over the voxels [c b, min(c b + c, n-1)]^3 (NaN if any
// voxel is NaN or infinite).
__global__ __launch_bounds__(64) void brick_max_kernel(const float4* __restrict__ vol, int nx, int ny, int nz, int bnx,
                                                       int bny, float2* __restrict__ out)
{
    const int b = blockIdx.x;
    const int bx = b % bnx, by = (b / bnx) % bny, bz = b / (bnx * bny);
    const int x0 = bx << kBrickShift, y0 = by << kBrickShift, z0 = bz << kBrickShift;
    const int ex = min(kBrickCells + 1, nx - x0), ey = min(kBrickCells + 1, ny - y0), ez = min(kBrickCells + 1, nz - z0);
    float m = -INFINITY, mc = -INFINITY;
    bool has_nan = false, has_nan_c = false;
    for (int t = threadIdx.x; t < ex * ey * ez; t += 64) {
        int lx = t % ex, ly = (t / ex) % ey, lz = t / (ex * ey);
        float4 v = vol[((size_t)(z0 + lz) * ny + (y0 + ly)) * nx + (x0 + lx)];
        // NaN or +-inf: samples next to such a voxel interpolate to NaN (inf * 0, inf - inf) whatever the others hold, and a
        // NaN density has a NaN opacity: the brick must stay active (a -inf would otherwise just lose the maximum)
        if (!(v.w - v.w == 0.0f)) has_nan = true;
        else if (v.w > m) m = v.w;
        if (v.x != v.x || v.y != v.y || v.z != v.z) has_nan_c = true;
        else mc = fmaxf(mc, fmaxf(v.x, fmaxf(v.y, v.z)));
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        m = fmaxf(m, __shfl_down(m, off, 64));
        mc = fmaxf(mc, __shfl_down(mc, off, 64));
        // (every lane takes part in every shuffle: behind a short-circuiting `||` a lane that has already seen a NaN would
        // sit the shuffle out, and the lane reading from it would get nothing -- the flag of a NaN found by any lane but
        // lane 0 was lost that way until round 2, and a brick holding nothing else but that voxel was skipped)
        const int other = __shfl_down((int)has_nan, off, 64), other_c = __shfl_down((int)has_nan_c, off, 64);
        has_nan = has_nan || other != 0;
        has_nan_c = has_nan_c || other_c != 0;
    }
    if (threadIdx.x == 0) out[b] = make_float2(has_nan ? NAN : m, has_nan_c ? NAN : mc);
}

// VOLUME_MASK looks at two volumes on one grid: record = (max density of the CT, max(r,g,b) of the mask)
__global__ void merge_bricks_kernel(const float2* __restrict__ density_vol, const float2* __restrict__ mask_vol,
                                    float2* __restrict__ out, int n)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = make_float2(density_vol[i].x, mask_vol[i].y);
}

// |v| above this (or NaN / inf) flags a range: b - a of two such values may overflow, and the lerp bound above needs it finite
constexpr float kProjRangeMag = 4.2535296e37f;  // 2^125

// One wavefront per brick of c = kBrickCells cells: (min, max) of .a over the voxels [c b, min(c b + c, n-1)]^3 -- the footprint of
// brick_max_kernel -- or (NaN, NaN) if any of them is NaN, infinite or above kProjRangeMag in magnitude.
__global__ __launch_bounds__(64) void brick_range_kernel(const float4* __restrict__ vol, int nx, int ny, int nz, int bnx, int bny,
                                                         float2* __restrict__ out)
{
    const int b = blockIdx.x;
    const int bx = b % bnx, by = (b / bnx) % bny, bz = b / (bnx * bny);
    const int x0 = bx << kBrickShift, y0 = by << kBrickShift, z0 = bz << kBrickShift;
    const int ex = min(kBrickCells + 1, nx - x0), ey = min(kBrickCells + 1, ny - y0), ez = min(kBrickCells + 1, nz - z0);
    float lo = INFINITY, hi = -INFINITY;
    int bad = 0;
    for (int t = threadIdx.x; t < ex * ey * ez; t += 64) {
        const int lx = t % ex, ly = (t / ex) % ey, lz = t / (ex * ey);
        const float a = vol[((size_t)(z0 + lz) * ny + (y0 + ly)) * nx + (x0 + lx)].w;
        if (!(fabsf(a) <= kProjRangeMag)) bad = 1;  // (NaN fails the comparison)
        else {
            lo = fminf(lo, a);
            hi = fmaxf(hi, a);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {  // (every lane takes part in every shuffle)
        lo = fminf(lo, __shfl_down(lo, off, 64));
        hi = fmaxf(hi, __shfl_down(hi, off, 64));
        bad |= __shfl_down(bad, off, 64);
    }
    if (threadIdx.x == 0) out[b] = bad ? make_float2(NAN, NAN) : make_float2(lo, hi);
}

// One workgroup: (min, max) over the n brick records into *out, (NaN, NaN) if any record is flagged.
__global__ __launch_bounds__(1024) void range_reduce_kernel(const float2* __restrict__ rec, int n, float2* __restrict__ out)
{
    __shared__ float s_lo[16], s_hi[16];
    __shared__ int s_bad[16];
    float lo = INFINITY, hi = -INFINITY;
    int bad = 0;
    for (int i = threadIdx.x; i < n; i += 1024) {
        const float2 r = rec[i];
        if (r.x != r.x || r.y != r.y) bad = 1;
        else {
            lo = fminf(lo, r.x);
            hi = fmaxf(hi, r.y);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        lo = fminf(lo, __shfl_down(lo, off, 64));
        hi = fmaxf(hi, __shfl_down(hi, off, 64));
        bad |= __shfl_down(bad, off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        s_lo[threadIdx.x >> 6] = lo;
        s_hi[threadIdx.x >> 6] = hi;
        s_bad[threadIdx.x >> 6] = bad;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 16; ++w) {
            lo = fminf(lo, s_lo[w]);
            hi = fmaxf(hi, s_hi[w]);
            bad |= s_bad[w];
        }
        *out = bad ? make_float2(NAN, NAN) : make_float2(lo, hi);
    }
}

}  // namespace vr
