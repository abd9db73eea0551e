// vr_bound.h -- per-pixel ray bounds (vr_set_ray_bounds, include/vr.h): the colour march of BASIC / LIGHT between two caller depth
// buffers.  Everything is the variant's own march (vr_kernels.h march_packet: positions, world positions, variable step, jitter, the
// clip box, the cut-off 0.95 / 1.0, fragment modes 1-4, the blend and the counters) except which in-box steps count: a step at p
// counts iff it passes IsInSampleCoords and S_near <= sigma(p) < S_far, with sigma(x) = (x.x*dir.x + x.y*dir.y) + x.z*dir.z and
// S_near / S_far = sigma of the bound's depth unprojected along the pixel's own ray set-up (ray placement: separately rounded in both
// arithmetic modes).  A step that does not count is a step outside the clip box: not fetched, not blended, not counted; p and w still
// advance by their rounded additions.  One lane per ray, one 8x8 packet per wavefront (map_pixel), on vr_ray.h's prologue and shell.
// Included by vr_launch.h once per arithmetic mode.
//
// The two buffers arrive in the .data members of the volume slots BASIC / LIGHT do not bind: MarchParams::vol[1].data = near,
// vol[2].data = far, W*H floats each, nullptr = no bound on that side (the host writes both members whatever the slots hold; the
// light volume travels in vol[1] the same way).  No field of MarchParams moves.
// The loop is shadow_packet's (LIGHT: fetch_rgba, world step, the packed shade and blend) and surf_packet's (BASIC: the density plane
// alone): the next step's corners are requested before this step's table texels are waited for, the distance-field byte is looked up
// two steps ahead, and with SKIP (flavour 27) a step in an inert brick of the variant's distance field loads nothing and a sample
// whose opacity is exactly 0 is not shaded -- both are the identity blend whether the step counts or not.
// sigma(p_k) does not decrease along a ray whose step size is not negative (each product is monotone -- p moves monotonically per
// component, dir has the step's signs -- and rounded sums of monotone terms are monotone): such a lane stops at the first step that
// fails the far test, and every lane walks the rounded additions up to its first step that passes the near test without a load.
// A lane with a NaN bound, or with S_far <= S_near, has no step that counts and issues no load at all.
//
// Registers (gfx950:xnack-, the project's flags, ROCm 7.2's hipcc; VGPRs / wavefronts per SIMD, no scratch anywhere): see DESIGN.md
// section 4.13; measure again with tools/isa_report.py before changing the loop's shape.
#pragma once
#include <type_traits>

namespace VR_KNS {

// sigma of include/vr.h: ray placement, summed left to right
__device__ __forceinline__ float bound_sigma(f3 x, f3 dir) { return (x.x * dir.x + x.y * dir.y) + x.z * dir.z; }

// S of depth d on the ray of pixel (px, py): setup_ray's pixel centre, unproject and world-to-uvw map
__device__ __forceinline__ float bound_s(const MarchParams& P, int px, int py, float d, f3 dir)
{
    const float fx = (float)px + 0.5f, fy = (float)py + 0.5f;
    const float ndcx = (2.0f * fx) / (float)P.W - 1.0f;
    const float ndcy = 1.0f - (2.0f * fy) / (float)P.H;
    const f3 g = unproject(P, ndcx, ndcy, d);
    return bound_sigma(mk3(g.x + 0.5f, g.y + 0.5f, 0.5f - 2.0f * g.z), dir);
}

// One ray: what a lane does for its pixel `slot` (V's march_packet between the bounds).
template <int V, bool OFF32, bool SKIP>
__device__ __forceinline__ void bound_packet(const MarchParams& P, const PixelSlot& slot, float4& dst, unsigned& blends, unsigned& covered,
                                             unsigned& fetched)
{
    static_assert(V == V_BASIC || V == V_LIGHT, "ray bounds exist for the unlit and the lit shader");
    constexpr bool kLit = V == V_LIGHT;
    using Corners = std::conditional_t<kLit, Fetch4, Fetch1>;
    RayStart r;
    // (covered: every pixel whose ray hits the box, as march_packet)
    covered = with_ray(P, slot, dst, r, [&]() __attribute__((always_inline)) {
        const float* d_near = reinterpret_cast<const float*>(P.vol[1].data);
        const float* d_far = reinterpret_cast<const float*>(P.vol[2].data);
        const bool has_near = d_near != nullptr, has_far = d_far != nullptr;  // (wave-uniform)
        const unsigned pixel = (unsigned)(slot.py * P.W + slot.px);          // (with_ray: the pixel is inside the viewport)
        float s_near = 0.0f, s_far = 0.0f;
        if (has_near) s_near = bound_s(P, slot.px, slot.py, d_near[pixel], r.dir);
        if (has_far) s_far = bound_s(P, slot.px, slot.py, d_far[pixel], r.dir);
        // no step can count: a NaN bound fails both comparisons, an empty interval has no sigma in it
        if ((has_near && !(s_near == s_near)) || (has_far && !(s_far == s_far)) || (has_near && has_far && s_far <= s_near)) return;
        const auto within = [&](f3 q) {
            const float sg = bound_sigma(q, r.dir);
            return (!has_near || sg >= s_near) && (!has_far || sg < s_far);
        };
        // sigma does not decrease from step to step unless the step size is negative (the variable step's never is)
        const bool far_ends = has_far && (P.toggle_varstep == 1 || P.step_size >= 0.0f);

        f3 p = r.p;
        [[maybe_unused]] f3 w = r.world0;
        const f3 step = r.step;
        [[maybe_unused]] const f3 wstep = world_step(P, r.dir);
        const int n_steps = P.steps_count;
        unsigned n = 0;
        int i = 0;
        // up to the near bound: the rounded additions alone
        if (has_near) {
            while (i < n_steps && !(bound_sigma(p, r.dir) >= s_near)) {
                p = mk3(p.x + step.x, p.y + step.y, p.z + step.z);
                if constexpr (kLit) w = mk3(w.x + wstep.x, w.y + wstep.y, w.z + wstep.z);
                ++i;
            }
        }

        // step i: corners of p in F (requested one iteration ago) when `have`; R = distance-field byte of p + step (requested one
        // iteration ago)
        Corners F;
        float fx = 0.0f, fy = 0.0f, fz = 0.0f;
        bool have = false;
        unsigned R = 0;
        if (i < n_steps && in_box(P, r, i, p) && within(p)) {
            have = !SKIP || dist_at(P, brick_of<OFF32>(P, p)) == 0u;
            if (have) {
                if constexpr (kLit) fetch_rgba<OFF32>(P.vol[0], p, F, fx, fy, fz);
                else fetch_a<OFF32>(P.vol[0], p, F, fx, fy, fz);
            }
        }
        if constexpr (SKIP) R = dist_at(P, brick_of<OFF32>(P, mk3(p.x + step.x, p.y + step.y, p.z + step.z)));
        for (; i < n_steps; ++i) {
            const bool inb = in_box(P, r, i, p);
            if (!inb && gone(P, step, p)) break;
            if (far_ends && !(bound_sigma(p, r.dir) < s_far)) break;  // no later step passes the far test
            const bool counts = inb && within(p);
            const f3 pn = mk3(p.x + step.x, p.y + step.y, p.z + step.z);
            // the next step: loaded unless it does not count or lies in an inert brick
            bool next = i + 1 < n_steps && in_box(P, r, i + 1, pn) && within(pn);
            if constexpr (SKIP) {
                next = next && R == 0u;
                R = dist_at(P, brick_of<OFF32>(P, mk3(pn.x + step.x, pn.y + step.y, pn.z + step.z)));  // (issued before the corners below)
            }
            // this step's sample: its table texels are requested before the next step's corners, so that waiting for them leaves
            // those eight loads in flight
            const bool sample = counts && have;
            bool shaded = false;
            v2f zw = v2f{0.0f, 0.0f}, gxy = zw;
            TfFetch tq = {};
            if (sample) {
                if constexpr (kLit) zw = interp_zw(F, fx, fy, fz);  // (gradient z, density)
                else zw.y = interp_a(F, fx, fy, fz);
                shaded = !SKIP || !opacity_is_zero(P, zw.y);
                if (shaded) {
                    tq = tf_fetch(P.tf[0], zw.y);
                    if constexpr (kLit) gxy = interp_xy(F, fx, fy, fz);
                }
            }
            Corners G;
            float gx = 0.0f, gy = 0.0f, gz = 0.0f;
            __builtin_amdgcn_sched_barrier(0);
            if (next) {
                if constexpr (kLit) fetch_rgba<OFF32>(P.vol[0], pn, G, gx, gy, gz);
                else fetch_a<OFF32>(P.vol[0], pn, G, gx, gy, gz);
            }
            __builtin_amdgcn_sched_barrier(0);
            if (counts) {
                ++n;
                if (sample) {
                    ++fetched;
                    if (shaded) {
                        if constexpr (kLit) {
                            light_shade_blend(P, w, zw, gxy, tq, dst);
                        } else {
                            const TfSample t = tf_finish(tq);
                            blend(t.rgb, t.opacity, dst);
                        }
                    }
                    if (!can_blend<V>(dst.w)) break;  // the cut-off: no later iteration can blend
                }
            }
            F = G;
            fx = gx;
            fy = gy;
            fz = gz;
            have = next;
            p = pn;
            if constexpr (kLit) w = mk3(w.x + wstep.x, w.y + wstep.y, w.z + wstep.z);
        }
        blends = n;
    });
}

template <int V, bool OFF32, bool SKIP, bool BATCH = false>
__global__ __launch_bounds__(64) void march_bound_kernel(const MarchBatch B)
{
    march_shell<BATCH>(B, [](auto&... a) { bound_packet<V, OFF32, SKIP>(a...); });
}

}  // namespace VR_KNS
