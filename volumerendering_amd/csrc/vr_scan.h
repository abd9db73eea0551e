// vr_scan.h -- the exclusive prefix scan of the voxel tools on the device: 32-bit counts in, the sums before each element out, a 64-bit
// total.  Hand-written, no library: sums per tile of kScanTile (scan_sums_kernel), one workgroup over the tile sums
// (scan_spine_kernel), add back (scan_apply_kernel).  The host launches the three through tool_scan (vr_api_tools.h); contour tracing
// (vr_outline.h), connected components (vr_comp.h) and surface extraction (vr_mesh.h) number their corners, runs, vertices and
// triangles with it.  Exact integer work: nothing can be fused, compiled once, in vr_api.hip alone.
#pragma once

namespace vr {

constexpr int kScanTile = 1024;  // elements per workgroup of a scan: four per lane

// ---- the scan ------------------------------------------------------------------------------------------------------------------------

// exclusive scan of one value per lane over the workgroup of 256; *total = the sum (every lane gets both)
__device__ __forceinline__ unsigned long long block_scan_256(unsigned long long v, unsigned long long* s, unsigned long long* total)
{
    const unsigned t = threadIdx.x;
    s[t] = v;
    __syncthreads();
    for (unsigned off = 1; off < 256u; off <<= 1) {
        const unsigned long long add = t >= off ? s[t - off] : 0ull;
        __syncthreads();
        s[t] += add;
        __syncthreads();
    }
    const unsigned long long incl = s[t];
    *total = s[255];
    __syncthreads();  // (s is free again)
    return incl - v;
}

__global__ __launch_bounds__(256) void scan_sums_kernel(const unsigned* in, unsigned long long n, unsigned long long* sums)
{
    __shared__ unsigned long long s[256];
    const unsigned long long i0 = (unsigned long long)blockIdx.x * kScanTile + threadIdx.x * 4u;
    unsigned long long v = 0ull;
    for (int e = 0; e < 4; ++e)
        if (i0 + e < n) v += in[i0 + e];
    unsigned long long total;
    (void)block_scan_256(v, s, &total);
    if (threadIdx.x == 0u) sums[blockIdx.x] = total;
}

// one workgroup: the tile sums become the sums before each tile, *total their sum
__global__ __launch_bounds__(256) void scan_spine_kernel(unsigned long long* sums, unsigned long long nb, unsigned long long* total)
{
    __shared__ unsigned long long s[256];
    unsigned long long carry = 0ull;
    for (unsigned long long b0 = 0; b0 < nb; b0 += 256u) {
        const unsigned long long i = b0 + threadIdx.x;
        const unsigned long long v = i < nb ? sums[i] : 0ull;
        unsigned long long chunk;
        const unsigned long long before = block_scan_256(v, s, &chunk);
        if (i < nb) sums[i] = carry + before;
        carry += chunk;
    }
    if (threadIdx.x == 0u) *total = carry;
}

// out[i] = the sum of in[0 .. i), its low 32 bits (the caller refuses a total beyond them); in == out is allowed
__global__ __launch_bounds__(256) void scan_apply_kernel(const unsigned* in, unsigned long long n, const unsigned long long* sums, unsigned* out)
{
    __shared__ unsigned long long s[256];
    const unsigned long long i0 = (unsigned long long)blockIdx.x * kScanTile + threadIdx.x * 4u;
    unsigned e4[4];
    unsigned long long v = 0ull;
    for (int e = 0; e < 4; ++e) {
        e4[e] = i0 + e < n ? in[i0 + e] : 0u;
        v += e4[e];
    }
    unsigned long long total;
    unsigned long long before = sums[blockIdx.x] + block_scan_256(v, s, &total);
    for (int e = 0; e < 4; ++e) {
        if (i0 + e < n) out[i0 + e] = (unsigned)before;
        before += e4[e];
    }
}

}  // namespace vr
