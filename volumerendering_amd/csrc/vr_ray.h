// vr_ray.h -- what the one-lane marches of vr_proj.h, vr_iso.h, vr_shadow.h, vr_surf.h and vr_bound.h share: the ray prologue (with_ray: BASIC's start,
// direction, step and the reference's quirks around them), the in-box and past-the-box tests of their step loops, and the kernel
// shell around a packet.  Each file keeps its own step loop: the loops differ in what is requested before the next step's corners.
// Included by vr_launch.h once per arithmetic mode, ahead of the five.
//
// Wave-uniform values (the clip bounds, steps_count, step_size) are read from MarchParams where they are used and never copied into
// RayStart: a copy in a per-lane struct moves them from SGPRs to VGPRs (march_proj_kernel: 59 -> 68 VGPRs, 8 -> 7 wavefronts per SIMD).
// Every VGPR figure in this file comes from a cross-compile for gfx950:xnack- with the project's flags on ROCm 7.2's hipcc; they
// explain the shapes below (the callback, always_inline, ClipBox by value).  Measure again with
// tools/isa_report.py before simplifying any of them.
#pragma once

namespace VR_KNS {

// A lane's ray as its step loop starts.
struct RayStart {
    f3 p;          // position of step 0 (jittered)
    f3 step;       // p += step, with the variable-step override
    f3 dir;
    f3 world0;     // LIGHT's world position of step 0
    int n_inside;  // steps [0, n_inside) are certainly inside IsInSampleCoords (steps_inside)
};

// Sets up the ray of pixel `slot`: fills r and calls march() when there is something to march; fragment modes 1-4 write dst instead.
// Returns whether the ray hits the box (also in the fragment modes).  march is a callback that reads the caller's r, and not code
// behind a returned flag or a callback that is handed r: either costs march_iso_kernel two VGPRs and with them a wavefront per SIMD
// (72 -> 74 in its batched 64-bit form).  The callers mark it always_inline, so that it is inlined as early as with_ray itself
// (march_surf_kernel's skipping 64-bit form: 72 VGPRs, 74 when the inliner gets to it later).
template <class F>
__device__ __forceinline__ bool with_ray(const MarchParams& P, const PixelSlot& slot, float4& dst, RayStart& r, F&& march)
{
    if (!(slot.active && slot.px >= P.rect[0] && slot.px <= P.rect[2] && slot.py >= P.rect[1] && slot.py <= P.rect[3])) return false;
    const Ray ray = setup_ray(P, slot.px, slot.py);
    if (!ray.hit) return false;
    const f3 diff = mk3(ray.end.x - ray.start.x, ray.end.y - ray.start.y, ray.end.z - ray.start.z);
    const f3 dir = normalize3s(diff);
    const float ray_len = length3s(diff);
    if (P.fragment_mode == 1) {
        dst = make_float4(fabsf(dir.x), fabsf(dir.y), fabsf(dir.z), 1.0f);
        return true;
    } else if (P.fragment_mode == 2) {
        dst = make_float4(ray.start.x, ray.start.y, ray.start.z, 1.0f);
        return true;
    } else if (P.fragment_mode == 3) {
        dst = make_float4(ray.end.x, ray.end.y, ray.end.z, 1.0f);
        return true;
    } else if (P.fragment_mode == 4) {
        dst = make_float4(0.5f * (ray.world0.x / 1.0f) + 0.5f, -0.5f * (ray.world0.y / 1.0f) + 0.5f, 0.0f, 1.0f);
        return true;
    }
    // the variable-step override comes after LIGHT's world step (world_step reads P.step_size), and jitter uses the overridden step
    float step_size = P.step_size;
    if (P.toggle_varstep == 1) step_size = ray_len / (float)P.steps_count;
    r.p = ray.start;
    if (P.toggle_jitter == 1) {
        const float j = jitter((float)slot.px + 0.5f, (float)slot.py + 0.5f);
        r.p = mk3(r.p.x + (dir.x * step_size) * j, r.p.y + (dir.y * step_size) * j, r.p.z + (dir.z * step_size) * j);
    }
    r.step = mk3(dir.x * step_size, dir.y * step_size, dir.z * step_size);
    r.dir = dir;
    r.world0 = ray.world0;
    r.n_inside = steps_inside(r.p, r.step, P.bmin[0], P.bmin[1], P.bmin[2], P.bmax[0], P.bmax[1], P.bmax[2]);
    march();
    return true;
}

// LIGHT's CalculateWorldStep: from the step size before the variable-step override
__device__ __forceinline__ f3 world_step(const MarchParams& P, f3 dir)
{
    f3 wstep = mk3(dir.x * (P.step_size * 1.0f), dir.y * (P.step_size * 1.0f), dir.z * (P.step_size * 0.5f));
    wstep.z = wstep.z * (-1.0f);
    return wstep;
}

// The clip bounds of IsInSampleCoords (wave-uniform), apart from the per-lane RayStart.  Filled member by member and handed on by
// value: the compiler then keeps the six in SGPRs as it does plain locals (by reference, or brace-initialised: VGPRs).
struct ClipBox {
    float x0, y0, z0, x1, y1, z1;
};
__device__ __forceinline__ ClipBox clip_box(const MarchParams& P)
{
    ClipBox b;
    b.x0 = P.bmin[0];
    b.y0 = P.bmin[1];
    b.z0 = P.bmin[2];
    b.x1 = P.bmax[0];
    b.y1 = P.bmax[1];
    b.z1 = P.bmax[2];
    return b;
}

// step i at q is inside IsInSampleCoords
__device__ __forceinline__ bool in_box(const ClipBox b, const RayStart& r, int i, f3 q)
{
    return i < r.n_inside || (q.x >= b.x0 && q.x <= b.x1 && q.y >= b.y0 && q.y <= b.y1 && q.z >= b.z0 && q.z <= b.z1);
}

// p moves monotonically per component: once past the far bound it never returns
__device__ __forceinline__ bool gone(const ClipBox b, f3 step, f3 p)
{
    const bool gone = (step.x >= 0.0f && p.x > b.x1) || (step.x <= 0.0f && p.x < b.x0) || (step.y >= 0.0f && p.y > b.y1) ||
                      (step.y <= 0.0f && p.y < b.y0) || (step.z >= 0.0f && p.z > b.z1) || (step.z <= 0.0f && p.z < b.z0);
    return gone;
}

// ... the same with the bounds read where they are tested, all six in front of the short-circuit chain (read behind its
// lane-divergent branches they end up in VGPRs: march_proj_kernel 62 -> 68).  vr_iso.h reads them once in front of its loop
// instead: that keeps iso_point_kernel's one-frame 32-bit form at 63 VGPRs (65 with these); in vr_proj.h it would cost four (62 -> 66).
__device__ __forceinline__ bool in_box(const MarchParams& P, const RayStart& r, int i, f3 q) { return in_box(clip_box(P), r, i, q); }
__device__ __forceinline__ bool gone(const MarchParams& P, f3 step, f3 p) { return gone(clip_box(P), step, p); }

// The kernel around a packet: the frame's parameters, the lane's pixel, packet(P, slot, dst, samples, covered, fetched), the store
// and the workgroup's record.
template <bool BATCH, class F>
__device__ __forceinline__ void march_shell(const MarchBatch& B, F&& packet)
{
    const MarchParams& P = frame_params<BATCH>(B);
    const unsigned long long t_start = wall_clock64();
    const PixelSlot slot = map_pixel(P);
    float4 dst = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    unsigned samples = 0, covered = 0, fetched = 0;
    packet(P, slot, dst, samples, covered, fetched);
    if (slot.active || (P.packed && slot.in_launch)) P.out[slot.out_index] = dst;
    store_block_counts(P, samples, covered, fetched, t_start);
}

}  // namespace VR_KNS
