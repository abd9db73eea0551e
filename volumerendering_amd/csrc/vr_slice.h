// vr_slice.h -- slice views of one volume slot (vr_slice_async, include/vr.h): parallel sample lines on a caller-defined plane instead
// of the viewport's perspective rays.  Pixel (px, py) starts at b = (origin + px * du) + py * dv (texture space, separately rounded in
// both arithmetic modes: placement) and takes slab_steps positions p_0 = b, p_{k+1} = p_k + dn (rounded additions).  The positions
// inside the unit cube are sampled -- BASIC's trilinear .a fetch in the arithmetic mode, or the .a of the voxel tex3_nearest addresses
// -- and reduced to their maximum, minimum or mean exactly as the projections of vr_proj.h are; the value then goes through one TF slot
// and one FrontToBackBlend onto dst = 0.  The context's uniforms, clip box and viewport play no part: the kernel has a parameter
// struct of its own (SliceParams, vr_device.h) and none of map_pixel / with_ray / march_shell.
// One lane per output pixel, one 8x8 pixel tile per wavefront (and per workgroup): a tile's gathers stay within few bricks of the
// bricked copy whatever the plane's orientation.  Included by vr_launch.h once per arithmetic mode.
//
// The step loop has proj_packet's shape: the next step's loads are issued before this step is interpolated, and the brick record is
// looked up two steps ahead.  It leaves once p has passed the unit cube for good: positions are monotone per component (rounding is
// monotone), so a component beyond the face its dn points away from never returns; a NaN component stays NaN.
//
// Exact skipping (SKIP) by the sliced slot's range records -- (min .a, max .a) over the (c+1)^3 voxels a brick of c^3 base cells can
// touch, (NaN, NaN) when flagged (brick_range_kernel, vr_prep.h) -- with vr_proj.h's rules and early exit, whose header proves that a
// brick's range bounds every trilinear sample whose base cell lies in it.
// NEAREST reads the record of the same brick, the brick of p's BASE cell t = clamp(floor(p * n - 0.5), 0, n - 1) per axis, and that
// brick bounds the voxel i = clamp(floor(p * n), 0, n - 1) it addresses, because i is t or t + 1 and brick b = t >> 2 covers the voxels
// 4 b .. min(4 b + 4, n - 1):
//   x' = fl(p * n) is in [0, n] for a counted p (p in [0, 1]); floor(x') = i before the clamp.
//   Separate rounding: the base coordinate is fl(x' - 0.5), and x' - 0.5 is exact for x' >= 0.25 (Sterbenz below 1; above, 0.5 is a
//     multiple of ulp(x') since n < 2^16), so floor of it is i - 1 or i.  x' < 0.25 gives a negative coordinate: t clamps to 0 = i.
//   Fused: the base coordinate is fl(z - 0.5) with z = p * n exact.  Rounding is monotone and moves a value across an integer only
//     onto it: if fl(z) was rounded up to the integer k then i = k and z - 0.5 lies just below k - 0.5, t = k - 1; if fl(z - 0.5)
//     was rounded up to k then z lies just below k + 0.5 and i = k = t; otherwise i - t = floor(z) - floor(z - 0.5), 0 or 1.
//   At the far face x' = n: i clamps to n - 1 and t = floor(n - 0.5) = n - 1.  (Checked by an adversarial search in both modes:
//   tests/test_slice.py.)
// So the voxel's value lies in [rec.x, rec.y], and a flagged record (NaN voxel, infinity) is never skipped.
//
// Counters: every wavefront stores its three sums (counted samples, pixels with n > 0, samples loaded) with plain stores;
// slice_sum_kernel (vr_frame.h) adds them up when vr_slice_counters asks.
#pragma once

namespace VR_KNS {

__device__ __forceinline__ bool slice_in_cube(f3 p)
{
    return p.x >= 0.0f && p.x <= 1.0f && p.y >= 0.0f && p.y <= 1.0f && p.z >= 0.0f && p.z <= 1.0f;  // (NaN fails)
}

// p has left the unit cube for good
__device__ __forceinline__ bool slice_gone(f3 dn, f3 p)
{
    return (dn.x >= 0.0f && p.x > 1.0f) || (dn.x <= 0.0f && p.x < 0.0f) || (dn.y >= 0.0f && p.y > 1.0f) || (dn.y <= 0.0f && p.y < 0.0f) ||
           (dn.z >= 0.0f && p.z > 1.0f) || (dn.z <= 0.0f && p.z < 0.0f) || p.x != p.x || p.y != p.y || p.z != p.z;
}

// record of the brick of p's base cell: brick_of / brick_record (vr_kernels.h) on the slice's own grid
__device__ __forceinline__ float2 slice_record(const SliceParams& S, f3 p)
{
    const int bx = (int)__builtin_amdgcn_fmed3f(mad(p.x, S.bsx, -kBrickHalf), 0.0f, (float)(S.bnx - 1));
    const int by = (int)__builtin_amdgcn_fmed3f(mad(p.y, S.bsy, -kBrickHalf), 0.0f, (float)(S.bny - 1));
    const int bz = (int)__builtin_amdgcn_fmed3f(mad(p.z, S.bsz, -kBrickHalf), 0.0f, (float)(S.bnz - 1));
    const int bid = __mul24(__mul24(bz, S.bny) + by, S.bnx) + bx;
    return *reinterpret_cast<const float2*>(reinterpret_cast<const char*>(S.bricks) + ((unsigned)bid << 3));
}

// slot of the voxel tex3_nearest addresses
__device__ __forceinline__ unsigned slice_nearest_slot(const DevVolume& v, f3 p)
{
    const int i = clampi((int)floorf(p.x * (float)v.nx), 0, v.nx - 1);
    const int j = clampi((int)floorf(p.y * (float)v.ny), 0, v.ny - 1);
    const int k = clampi((int)floorf(p.z * (float)v.nz), 0, v.nz - 1);
    if (v.bricked)
        return ((unsigned)i >> kVbS) * kVbN + ((unsigned)i & kVbM) + ((unsigned)j >> kVbS) * v.brick_row + (((unsigned)j & kVbM) << kVbS) +
               ((unsigned)k >> kVbS) * v.brick_slab + (((unsigned)k & kVbM) << (2u * kVbS));
    return ((unsigned)k * (unsigned)v.ny + (unsigned)j) * (unsigned)v.nx + (unsigned)i;
}

// the loads of one sample (NEAREST: one voxel, in q.a) and its value once they have arrived
template <bool NEAREST, bool OFF32>
__device__ __forceinline__ void slice_fetch(const DevVolume& v, f3 p, Fetch1& q, float& fx, float& fy, float& fz)
{
    if constexpr (NEAREST) q.a = load_a<OFF32>(v, slice_nearest_slot(v, p));
    else fetch_a<OFF32>(v, p, q, fx, fy, fz);
}
template <bool NEAREST>
__device__ __forceinline__ float slice_value(const Fetch1& q, float fx, float fy, float fz)
{
    if constexpr (NEAREST) return q.a;
    else return interp_a(q, fx, fy, fz);
}

// present_kernel's arithmetic (vr_frame.h) on one fragment
__device__ __forceinline__ unsigned slice_unorm8(float v)
{
    if (!(v > 0.0f)) v = 0.0f;
    if (v > 1.0f) v = 1.0f;
    return (unsigned)floorf(v * 255.0f + 0.5f);
}
__device__ __forceinline__ unsigned slice_present(float4 s)
{
    const float a = s.w;
    const float r = s.x * a + 1.0f * (1.0f - a);
    const float g = s.y * a + 1.0f * (1.0f - a);
    const float b = s.z * a + 1.0f * (1.0f - a);
    const float oa = s.w * a + 1.0f * (1.0f - a);
    return slice_unorm8(b) | (slice_unorm8(g) << 8) | (slice_unorm8(r) << 16) | (slice_unorm8(oa) << 24);
}

template <int REDUCE, bool NEAREST, bool OFF32, bool SKIP>
__global__ __launch_bounds__(64) void slice_kernel(const SliceParams S)
{
    const int tile = (int)blockIdx.x;
    const int ty = tile / S.tiles_x, tx = tile - ty * S.tiles_x;
    const int px = (tx << 3) + (int)(threadIdx.x & 7u), py = (ty << 3) + (int)(threadIdx.x >> 3);
    const bool active = px < S.width && py < S.height;
    float4 dst = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    unsigned n = 0, fetched = 0;
    if (active) {
        const f3 dn = mk3(S.dn[0], S.dn[1], S.dn[2]);
        f3 p = mk3((S.origin[0] + (float)px * S.du[0]) + (float)py * S.dv[0], (S.origin[1] + (float)px * S.du[1]) + (float)py * S.dv[1],
                   (S.origin[2] + (float)px * S.du[2]) + (float)py * S.dv[2]);
        const int n_steps = S.slab_steps;
        float m = REDUCE == kProjMax ? -INFINITY : (REDUCE == kProjMin ? INFINITY : 0.0f);
        float lim = 0.0f;  // early exit: MAX m >= lim, MIN m <= lim (NaN: never)
        if constexpr (SKIP && REDUCE != kProjAvg) lim = REDUCE == kProjMax ? S.vrange->y : S.vrange->x;
        bool done = false;

        // step i: the loads of p in F (requested one iteration ago) when `have`; R = record of p + dn (requested one iteration ago)
        Fetch1 F;
        float fx = 0.0f, fy = 0.0f, fz = 0.0f;
        bool have = false;
        float2 R = make_float2(0.0f, 0.0f);
        if (slice_in_cube(p)) {
            have = !SKIP || !proj_inert<REDUCE>(slice_record(S, p), m);
            if (have) slice_fetch<NEAREST, OFF32>(S.vol, p, F, fx, fy, fz);
        }
        if constexpr (SKIP) R = slice_record(S, mk3(p.x + dn.x, p.y + dn.y, p.z + dn.z));
        for (int i = 0; i < n_steps; ++i) {
            const bool inb = slice_in_cube(p);
            if (!inb && slice_gone(dn, p)) break;
            const f3 pn = mk3(p.x + dn.x, p.y + dn.y, p.z + dn.z);
            // the next step: loaded unless it is outside the cube or its brick cannot change m as m stands now (m only ever moves
            // towards the side that makes more bricks inert: the test stays true when it is applied one step early)
            bool next = i + 1 < n_steps && !done && slice_in_cube(pn);
            if constexpr (SKIP) {
                next = next && !proj_inert<REDUCE>(R, m);
                R = slice_record(S, mk3(pn.x + dn.x, pn.y + dn.y, pn.z + dn.z));  // (issued before the loads below)
            }
            Fetch1 G;
            float gx = 0.0f, gy = 0.0f, gz = 0.0f;
            __builtin_amdgcn_sched_barrier(0);
            if (next) slice_fetch<NEAREST, OFF32>(S.vol, pn, G, gx, gy, gz);
            __builtin_amdgcn_sched_barrier(0);
            if (inb) {
                ++n;
                if (have) {
                    proj_update<REDUCE>(m, slice_value<NEAREST>(F, fx, fy, fz));
                    ++fetched;
                    if constexpr (SKIP && REDUCE == kProjMax) done = m >= lim;
                    if constexpr (SKIP && REDUCE == kProjMin) done = m <= lim;
                }
            }
            F = G;
            fx = gx;
            fy = gy;
            fz = gz;
            have = next;
            p = pn;
        }
        if (n != 0) {
            float v = m;
            if constexpr (REDUCE == kProjAvg) v = m / (float)n;
            const TfSample t = tf_lookup(S.tf, v);
            blend(t.rgb, t.opacity, dst);
        }
        const size_t o = (size_t)py * (size_t)S.width + (size_t)px;
        if (S.format == 1) reinterpret_cast<unsigned*>(S.out)[o] = slice_present(dst);
        else reinterpret_cast<float4*>(S.out)[o] = dst;
    }
    // the wavefront's record (every lane takes part in every shuffle)
    unsigned long long cn = n, cc = n != 0 ? 1u : 0u, cf = fetched;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        cn += __shfl_down(cn, off, 64);
        cc += __shfl_down(cc, off, 64);
        cf += __shfl_down(cf, off, 64);
    }
    if (threadIdx.x == 0) {
        unsigned long long* o = S.counts + (size_t)blockIdx.x * 3;
        o[0] = cn;
        o[1] = cc;
        o[2] = cf;
    }
}

}  // namespace VR_KNS
