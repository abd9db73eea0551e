// vr_surf.h -- the surface-position output of the unlit / lit shader (vr_set_output(VR_OUTPUT_SURFACE), include/vr.h): BASIC's march
// (same start, direction, steps, step size, variable step, jitter and rounded additions p += step) that accumulates the alpha line of
// FrontToBackBlend alone, a = mad(1 - a, o, a) with o = BASIC's opacity look-up of the density, and stops at the first in-box step
// after whose blend a > tau (MarchParams::iso carries tau: these launches read no level).  The surface is placed between that step and
// the one before it by the isosurface's rule on alpha, and the pixel is (q, a).  One lane per ray, one 8x8 packet per wavefront
// (map_pixel: launch order, packed tiles, the (frame, packet) items of batched launches).  Included by vr_launch.h once per arithmetic
// mode.
//
// What a step reads: the scalar density plane (4 bytes per corner, tex3_a's sampler in every layout) and two opacity texels.  No
// gradient, no colour table, no light.
// Exact skipping (SKIP, flavour 25): a step whose base cell lies in a brick that BASIC's distance field marks inert (byte != 0) has
// opacity exactly +-0 -- the field's own guarantee, which rests on the opacity table's zero prefix alone -- so mad(1 - a, +-0, a) == a
// in both arithmetic modes (a starts at +0 and never becomes -0): nothing is loaded, and the step cannot be the hit.  Because a does
// not change there, a_prev of the hit step is known without a second fetch.
// Early exit: a lane stops at its hit (or at a NaN alpha) and issues no further loads; the wavefront ends when its last lane has hit
// or left the box.
// The loop issues the corner loads of the next step before it waits for this step's opacity texels, and looks each distance-field
// byte up two steps ahead, so that waiting for a byte never waits for the corners still in flight (loads complete in order).
//
// (The depth a rasteriser drawing at q would write, vr_surface_depth_async: surface_depth_kernel, vr_frame.h.)
#pragma once

namespace VR_KNS {

// One ray: what a lane does for its pixel `slot`.
template <bool OFF32, bool SKIP>
__device__ __forceinline__ void surf_packet(const MarchParams& P, const PixelSlot& slot, float4& dst, unsigned& samples, unsigned& covered,
                                            unsigned& fetched)
{
    RayStart r;
    with_ray(P, slot, dst, r, [&]() __attribute__((always_inline)) {
        f3 p = r.p;
        const f3 step = r.step;
        const float tau = P.iso;
        const int n_steps = P.steps_count;
        unsigned n = 0;
        float a = 0.0f, a_prev = 0.0f;
        f3 pp = p;  // the step before the current one, and whether it was in the box
        bool prev_inb = false;
        bool hit = false;

        // step i: corners of p in F (requested one iteration ago) when `have`; R = distance-field byte of p + step (requested one
        // iteration ago)
        Fetch1 F;
        float fx = 0.0f, fy = 0.0f, fz = 0.0f;
        bool have = false;
        unsigned R = 0;
        if (n_steps > 0 && in_box(P, r, 0, p)) {
            have = !SKIP || dist_at(P, brick_of<OFF32>(P, p)) == 0u;
            if (have) fetch_a<OFF32>(P.vol[0], p, F, fx, fy, fz);
        }
        if constexpr (SKIP) R = dist_at(P, brick_of<OFF32>(P, mk3(p.x + step.x, p.y + step.y, p.z + step.z)));
        for (int i = 0; i < n_steps; ++i) {
            const bool inb = in_box(P, r, i, p);
            if (!inb && gone(P, step, p)) break;
            const f3 pn = mk3(p.x + step.x, p.y + step.y, p.z + step.z);
            // the next step: loaded unless it is outside the box or in an inert brick
            bool next = i + 1 < n_steps && in_box(P, r, i + 1, pn);
            if constexpr (SKIP) {
                next = next && R == 0u;
                R = dist_at(P, brick_of<OFF32>(P, mk3(pn.x + step.x, pn.y + step.y, pn.z + step.z)));  // (issued before the corners below)
            }
            // this step's opacity texels are requested before the next step's corners, so that waiting for them leaves those eight
            // loads in flight
            const bool sample = inb && have;
            float o0 = 0.0f, o1 = 0.0f, fo = 0.0f;
            if (sample) {
                const float d = interp_a(F, fx, fy, fz);
                const float xo = mad(d, (float)P.tf[0].res_o, -0.5f);
                const float xo0 = floorf(xo);
                fo = xo - xo0;
                const int jo = padded_texel(xo0, P.tf[0].res_o);
                const float* po = reinterpret_cast<const float*>(reinterpret_cast<const char*>(P.tf[0].opacity) + ((unsigned)jo << 2));
                o0 = po[0];
                o1 = po[1];
            }
            Fetch1 G;
            float gx = 0.0f, gy = 0.0f, gz = 0.0f;
            __builtin_amdgcn_sched_barrier(0);
            if (next) fetch_a<OFF32>(P.vol[0], pn, G, gx, gy, gz);
            __builtin_amdgcn_sched_barrier(0);
            if (inb) {
                ++n;
                if (sample) {
                    ++fetched;
                    a_prev = a;
                    a = mad(1.0f - a, lerpf(o0, o1, fo), a);  // the alpha line of FrontToBackBlend
                    if (a > tau) {
                        hit = true;
                        break;
                    }
                    if (!(a <= tau)) break;  // (a NaN alpha ends the loop and is no hit)
                }
            }
            pp = p;
            prev_inb = inb;
            F = G;
            fx = gx;
            fy = gy;
            fz = gz;
            have = next;
            p = pn;
        }
        samples = n;
        if (!hit) {
            dst = make_float4(0.0f, 0.0f, 0.0f, a);
            return;
        }
        covered = 1;
        // the surface point: p_k, or the isosurface's secant step on alpha from the previous in-box step
        f3 q = p;
        if (prev_inb) {
            const float t = (tau - a_prev) / (a - a_prev);
            if (t >= 0.0f && t <= 1.0f) q = mk3(mad(step.x, t, pp.x), mad(step.y, t, pp.y), mad(step.z, t, pp.z));
        }
        dst = make_float4(q.x, q.y, q.z, a);
    });
}

template <bool OFF32, bool SKIP, bool BATCH = false>
__global__ __launch_bounds__(64) void march_surf_kernel(const MarchBatch B)
{
    march_shell<BATCH>(B, [](auto&... a) { surf_packet<OFF32, SKIP>(a...); });
}

}  // namespace VR_KNS
