// vr_frame.h -- what happens to a frame around a march launch: the sums of its block counters, the launch order of the next one and
// the launch's measured span, the output merge (present) and the un-permute of gathered tiles, the depth of a surface frame, the
// counter sums of a slice view, and the spin that vr_stream() probes the hardware queues with.  Kernels that exist once, in namespace
// vr; only the C ABI's translation unit (vr_api.hip) includes them.
//   present_kernel   output merge PipelineBuilder.cpp:142-147 over fullscreen.wgsl:33-41 white, BGRA8Unorm
#pragma once
#include "vr_device.h"
#include "vr_shared.h"  // mat4_mul_point

namespace vr {

// ------------------------------------------------------------------------------------------------ present and tile unpack
__device__ __forceinline__ unsigned unorm8(float v)
{
    if (!(v > 0.0f)) v = 0.0f;
    if (v > 1.0f) v = 1.0f;
    return (unsigned)floorf(v * 255.0f + 0.5f);
}

// Output merge over the white background, BGRA8Unorm (PipelineBuilder.cpp:142-147, fullscreen.wgsl:33-41).
__global__ void present_kernel(const float4* __restrict__ frag, uint32_t* __restrict__ bgra, int n)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float4 s = frag[i];
    float a = s.w;
    float r = s.x * a + 1.0f * (1.0f - a);
    float g = s.y * a + 1.0f * (1.0f - a);
    float b = s.z * a + 1.0f * (1.0f - a);
    float oa = s.w * a + 1.0f * (1.0f - a);
    bgra[i] = unorm8(b) | (unorm8(g) << 8) | (unorm8(r) << 16) | (unorm8(oa) << 24);
}

// present_kernel reading the frame THROUGH the tile permutation: the root of the multi-GPU gather presents straight from the
// gathered, tile-major segments (gathered[r][n][64*64]), no assembled float frame in between (16 B read + 4 B written per
// pixel instead of an un-permute pass of 16 + 16 and a present pass of 16 + 4).  Same arithmetic as present_kernel.
__global__ void present_tiles_kernel(const float4* __restrict__ gathered, uint32_t* __restrict__ bgra, int W, int H, int tiles_x,
                                     int world, int tiles_per_rank_max)
{
    int x = blockIdx.x * blockDim.x + threadIdx.x;
    int y = blockIdx.y * blockDim.y + threadIdx.y;
    if (x >= W || y >= H) return;
    int t = (y / kTile) * tiles_x + (x / kTile);
    int r = t % world, n = t / world;
    size_t src = ((size_t)r * tiles_per_rank_max + n) * (kTile * kTile) + (y % kTile) * kTile + (x % kTile);
    float4 s = gathered[src];
    float a = s.w;
    float rr = s.x * a + 1.0f * (1.0f - a);
    float g = s.y * a + 1.0f * (1.0f - a);
    float b = s.z * a + 1.0f * (1.0f - a);
    float oa = s.w * a + 1.0f * (1.0f - a);
    bgra[(size_t)y * W + x] = unorm8(b) | (unorm8(g) << 8) | (unorm8(rr) << 16) | (unorm8(oa) << 24);
}

// Root side of the image-tile gather: gathered[r][n][64*64] -> frame[y*W+x]
__global__ void unpack_tiles_kernel(const float4* __restrict__ gathered, float4* __restrict__ frame, int W, int H,
                                    int tiles_x, int world, int tiles_per_rank_max)
{
    int x = blockIdx.x * blockDim.x + threadIdx.x;
    int y = blockIdx.y * blockDim.y + threadIdx.y;
    if (x >= W || y >= H) return;
    int t = (y / kTile) * tiles_x + (x / kTile);
    int r = t % world, n = t / world;
    size_t src = ((size_t)r * tiles_per_rank_max + n) * (kTile * kTile) + (y % kTile) * kTile + (x % kTile);
    frame[(size_t)y * W + x] = gathered[src];
}

// ... and the same un-permute for tiles that were presented where they were rendered (4 B per pixel: the multi-GPU loop gathers
// BGRA8 tiles instead of float tiles when only the presented frame is wanted)
__global__ void unpack_tiles_u32_kernel(const uint32_t* __restrict__ gathered, uint32_t* __restrict__ frame, int W, int H, int tiles_x,
                                        int world, int tiles_per_rank_max)
{
    int x = blockIdx.x * blockDim.x + threadIdx.x;
    int y = blockIdx.y * blockDim.y + threadIdx.y;
    if (x >= W || y >= H) return;
    int t = (y / kTile) * tiles_x + (x / kTile);
    int r = t % world, n = t / world;
    size_t src = ((size_t)r * tiles_per_rank_max + n) * (kTile * kTile) + (y % kTile) * kTile + (x % kTile);
    frame[(size_t)y * W + x] = gathered[src];
}

// ------------------------------------------------------------------------------------------------ behind a launch: counters, order, span
// One block: adds the per-block counts of the last march launch up (out[0..2]).
__global__ __launch_bounds__(256) void sum_block_counts_kernel(const unsigned long long* __restrict__ in, int n_blocks,
                                                               unsigned long long* __restrict__ out)
{
    __shared__ unsigned long long part[4][3];
    unsigned long long a = 0, b = 0, f = 0;
    for (int i = threadIdx.x; i < n_blocks; i += 256) {
        a += in[(size_t)i * kBlockRecord];
        b += in[(size_t)i * kBlockRecord + 1];
        f += in[(size_t)i * kBlockRecord + 2];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        a += __shfl_down(a, off, 64);
        b += __shfl_down(b, off, 64);
        f += __shfl_down(f, off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        part[threadIdx.x >> 6][0] = a;
        part[threadIdx.x >> 6][1] = b;
        part[threadIdx.x >> 6][2] = f;
    }
    __syncthreads();
    if (threadIdx.x < 3) out[threadIdx.x] = part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
}

// One wavefront that stays busy for `ticks` of the 100 MHz clock (bounded): vr_stream()'s probe for streams that really
// run side by side (HIP maps streams onto a few hardware queues; two streams on one queue serialise).
__global__ __launch_bounds__(64) void spin_kernel(unsigned long long ticks, unsigned* __restrict__ sink)
{
    const unsigned long long t0 = wall_clock64();
    unsigned n = 0;
    while (wall_clock64() - t0 < ticks && n < 4000000u) {
        __builtin_amdgcn_s_sleep(8);
        ++n;
    }
    if (sink && threadIdx.x == 0 && n == 0xFFFFFFFFu) *sink = n;  // (never true: keeps the loop observable)
}

// One workgroup: order[] = the logical blocks of the launch whose records are `in`, sorted by the longest per-ray sample
// chain of the block (record word 5, bits 40..), longest first, SEPARATELY within each residue class of the block index
// modulo 8: position b of the order holds a block lb with lb % 8 == b % 8.  Workgroups are dispatched round-robin over the
// 8 XCDs, so a block stays on the XCD its index maps to (what map_pixel relies on) and every XCD runs its own
// blocks longest-processing-time-first.  Eight counting sorts over 128 key buckets each (n_blocks % 8 == 0).
// It also reports how long the launch took: last workgroup end - first workgroup start of the records it reads (100 MHz
// ticks, to host-visible memory; vr_kernel_times).  Timing events around every launch cost the frame's stream 11 us.
// pw_heads: the queue heads of the persistent-wavefront launch whose records these are (vr_pw.h) -- cleared here, behind that
// launch, for the next launch that uses the slot.
__global__ __launch_bounds__(1024) void order_blocks_kernel(const unsigned long long* __restrict__ in, int n_blocks,
                                                            unsigned* __restrict__ order, unsigned* __restrict__ longest_chain,
                                                            unsigned long long* __restrict__ span_ticks,
                                                            unsigned* __restrict__ pw_heads,
                                                            unsigned long long* __restrict__ end_tick = nullptr)
{
    if (pw_heads != nullptr && threadIdx.x < 8) pw_heads[threadIdx.x * 64] = 0u;
    __shared__ unsigned hist[1024];  // [class 0..7][bucket 0..127]
    __shared__ unsigned base[1024];
    __shared__ unsigned chain_max;
    __shared__ unsigned long long t_first, t_last;
    const int t = threadIdx.x;
    hist[t] = 0;
    if (t == 0) {
        chain_max = 0;
        t_first = ~0ull;
        t_last = 0ull;
    }
    unsigned my_chain = 0;
    unsigned long long my_first = ~0ull, my_last = 0ull;
    __syncthreads();
    // every record is read ONCE (a launch that recycles the record buffer under this kernel can then only change the
    // order, never make it something other than a permutation); bucket 0 = the longest chains (32 steps per bucket)
    unsigned short bk[kOrderMaxBlocks / 1024];  // (private memory: the loops are not unrolled)
    for (int k = 0; k * 1024 < n_blocks; ++k) {
        const int b = t + k * 1024;
        if (b < n_blocks) {
            const unsigned long long crit = in[(size_t)b * kBlockRecord + 5] >> 40;
            const unsigned long long b0 = in[(size_t)b * kBlockRecord + 3], b1 = in[(size_t)b * kBlockRecord + 4];
            my_first = b0 < my_first ? b0 : my_first;
            my_last = b1 > my_last ? b1 : my_last;
            my_chain = crit > my_chain ? (unsigned)crit : my_chain;
            const unsigned q = (unsigned)(crit >> 5);
            bk[k] = (unsigned short)(((unsigned)b & 7u) * 128u + (127u - (q > 127u ? 127u : q)));
            atomicAdd(&hist[bk[k]], 1u);
        }
    }
    __syncthreads();
    {   // exclusive prefix sum inside each class: classes are 128 consecutive entries = two wavefronts
        const unsigned mine = hist[t];
        unsigned incl = mine;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned up = (unsigned)__shfl_up((int)incl, off, 64);
            if ((t & 63) >= off) incl += up;
        }
        __shared__ unsigned wave_total[16];
        if ((t & 63) == 63) wave_total[t >> 6] = incl;
        __syncthreads();
        const unsigned before = ((t >> 6) & 1) ? wave_total[(t >> 6) - 1] : 0u;  // the class's first wavefront
        base[t] = before + incl - mine;
    }
    __syncthreads();
    // the launch's longest ray chain + 1 (0 = not written yet), to host-visible memory: the host's choice of lanes per ray for
    // a later launch of the same shape reads it without synchronising (vr_api.hip, enqueue_render)
    if (longest_chain) {
        atomicMax(&chain_max, my_chain);
        __syncthreads();
        if (t == 0) *longest_chain = chain_max + 1u;
    }
    if (span_ticks) {
        // (a launch of several frames: the first frame's records stand for all of them -- the frames' workgroups are
        // interleaved, so its first start and last end are the launch's to within a few workgroup times)
        atomicMin(&t_first, my_first);
        atomicMax(&t_last, my_last);
        __syncthreads();
        if (t == 0) {
            if (end_tick) *end_tick = t_last | 1ull;  // (the last workgroup's end on the device clock; before the span: the host reads the span first)
            __threadfence_system();
            *span_ticks = t_last >= t_first ? t_last - t_first + 1ull : 1ull;  // (0 = not written yet)
        }
    }
    // scatter with one cursor per (class, bucket): the i-th block of class x goes to position 8 * i + x
    for (int k = 0; k * 1024 < n_blocks; ++k) {
        const int b = t + k * 1024;
        if (b < n_blocks) order[8u * atomicAdd(&base[bk[k]], 1u) + ((unsigned)b & 7u)] = (unsigned)b;
    }
}

// Depth of a surface frame (vr_surface_depth_async): .w > tau false -> 1.0f; else q -> world (the inverse of setup_ray's
// world-to-uvw map) -> eye -> clip with the ray set-up's matrix product (separately rounded), depth = clip.z / clip.w.
struct DepthParams {
    float view[16], proj[16];
    float tau;
};
__global__ __launch_bounds__(256) void surface_depth_kernel(const float4* __restrict__ surf, float* __restrict__ depth, int n, const DepthParams D)
{
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= n) return;
    const float4 s = surf[i];
    float z = 1.0f;
    if (s.w > D.tau) {
        float e[4], c[4];
        mat4_mul_point(D.view, s.x - 0.5f, s.y - 0.5f, (0.5f - s.z) * 0.5f, 1.0f, e);
        mat4_mul_point(D.proj, e[0], e[1], e[2], e[3], c);
        z = c[2] / c[3];
    }
    depth[i] = z;
}

// One workgroup: adds the n wavefront records of a slice launch up (out[0..2]).
__global__ __launch_bounds__(1024) void slice_sum_kernel(const unsigned long long* __restrict__ in, unsigned n, unsigned long long* __restrict__ out)
{
    __shared__ unsigned long long part[16][3];
    unsigned long long a = 0, b = 0, f = 0;
    for (unsigned i = threadIdx.x; i < n; i += 1024u) {
        a += in[(size_t)i * 3];
        b += in[(size_t)i * 3 + 1];
        f += in[(size_t)i * 3 + 2];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        a += __shfl_down(a, off, 64);
        b += __shfl_down(b, off, 64);
        f += __shfl_down(f, off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        part[threadIdx.x >> 6][0] = a;
        part[threadIdx.x >> 6][1] = b;
        part[threadIdx.x >> 6][2] = f;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        unsigned long long s = 0;
        for (int w = 0; w < 16; ++w) s += part[w][threadIdx.x];
        out[threadIdx.x] = s;
    }
}

}  // namespace vr
