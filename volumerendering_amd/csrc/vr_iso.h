// vr_iso.h -- the shaded isosurface of volume slot 0 (VR_VARIANT_ISO, include/vr.h): the BASIC shader's march (same start,
// direction, steps, step size, variable step, jitter and rounded additions p += step) with LIGHT's world position beside it, stopped
// at the first sample inside IsInSampleCoords whose density is >= the level (MarchParams::iso).  The surface is placed between that
// sample and the one before it by one secant step, shaded there with LIGHT's BlinnPhong on the voxels' gradient, coloured by TF
// slot 0 at the level and blended once, opaque, onto dst = 0.  One lane per ray, one 8x8 packet per wavefront (map_pixel: launch
// order, packed tiles, the (frame, packet) items of batched launches).  Included by vr_launch.h once per arithmetic mode.
//
// Exact skipping (SKIP, flavour 21): a step whose base cell lies in a brick (brick_of) with record max < iso loads nothing.  The
// records are the projections' (brick_range_kernel, vr_prep.h): (min .a, max .a) over the voxels the brick's cells can touch, and
// vr_proj.h's header shows that a trilinear sample never exceeds the largest of its corners, in either arithmetic mode -- so such a
// step's density is < iso and it cannot be the hit.  The comparison is strict (a sample equal to the level is a hit), and a flagged
// (NaN, NaN) record fails it: never skipped.
// Early exit: a lane stops at its hit and issues no further loads; the wavefront ends when its last lane has hit or left the box.
// Hit tail: the secant step needs d at the previous in-box step.  When that step was skipped its density was never loaded: it is
// loaded now at the kept p_{k-1} -- the same operations, the same bits -- and its brick record guarantees it is finite and < iso.
// The loop issues the corner loads of the next step before it interpolates this one, and looks each brick record up two steps
// ahead, so that waiting for a record never waits for the corners still in flight (loads complete in order).
#pragma once

namespace VR_KNS {

// One ray: what a lane does for its pixel `slot`.
// SURF (vr_set_output(VR_OUTPUT_SURFACE)): the refined point is the pixel, (q, 1); nothing is shaded.
template <bool OFF32, bool SKIP, bool SURF = false>
__device__ __forceinline__ void iso_packet(const MarchParams& P, const PixelSlot& slot, float4& dst, unsigned& samples, unsigned& covered,
                                           unsigned& fetched)
{
    RayStart r;
    with_ray(P, slot, dst, r, [&]() __attribute__((always_inline)) {
        f3 p = r.p, w = r.world0;
        const f3 step = r.step, wstep = world_step(P, r.dir);
        const float iso = P.iso;
        const int n_steps = P.steps_count;
        const ClipBox box = clip_box(P);  // (read once, in front of the loop: vr_ray.h says why)
        unsigned n = 0;
        // the step before the current one: its position, world position, density (when loaded) and whether it was in the box
        f3 pp = p, wp = w;
        float dprev = 0.0f;
        bool prev_loaded = false, prev_inb = false;
        bool hit = false;
        float dk = 0.0f;

        // step i: corners of p in F (requested one iteration ago) when `have`; R = record of p + step (requested one iteration ago)
        Fetch1 F;
        float fx = 0.0f, fy = 0.0f, fz = 0.0f;
        bool have = false;
        float2 R = make_float2(0.0f, 0.0f);
        if (n_steps > 0 && in_box(box, r, 0, p)) {
            have = !SKIP || !(proj_record(P, p).y < iso);
            if (have) fetch_a<OFF32>(P.vol[0], p, F, fx, fy, fz);
        }
        if constexpr (SKIP) R = proj_record(P, mk3(p.x + step.x, p.y + step.y, p.z + step.z));
        for (int i = 0; i < n_steps; ++i) {
            const bool inb = in_box(box, r, i, p);
            if (!inb && gone(box, step, p)) break;
            const f3 pn = mk3(p.x + step.x, p.y + step.y, p.z + step.z);
            // the next step: loaded unless it is outside the box or its brick lies below the level
            bool next = i + 1 < n_steps && in_box(box, r, i + 1, pn);
            if constexpr (SKIP) {
                next = next && !(R.y < iso);
                R = proj_record(P, mk3(pn.x + step.x, pn.y + step.y, pn.z + step.z));  // (issued before the corners below)
            }
            Fetch1 G;
            float gx = 0.0f, gy = 0.0f, gz = 0.0f;
            __builtin_amdgcn_sched_barrier(0);
            if (next) fetch_a<OFF32>(P.vol[0], pn, G, gx, gy, gz);
            __builtin_amdgcn_sched_barrier(0);
            bool loaded = false;
            float d = 0.0f;
            if (inb) {
                ++n;
                if (have) {
                    d = interp_a(F, fx, fy, fz);
                    loaded = true;
                    ++fetched;
                    if (d >= iso) {  // (NaN never hits)
                        hit = true;
                        dk = d;
                        break;
                    }
                }
            }
            pp = p;
            wp = w;
            dprev = d;
            prev_loaded = loaded;
            prev_inb = inb;
            F = G;
            fx = gx;
            fy = gy;
            fz = gz;
            have = next;
            p = pn;
            w = mk3(w.x + wstep.x, w.y + wstep.y, w.z + wstep.z);
        }
        samples = n;
        if (!hit) return;
        covered = 1;
        // the surface point: p_k, or the secant step from the previous in-box step
        f3 q = p, wq = w;
        if (prev_inb) {
            const float d0 = prev_loaded ? dprev : tex3_a<OFF32>(P.vol[0], pp);
            const float t = (iso - d0) / (dk - d0);
            if (t >= 0.0f && t <= 1.0f) {
                q = mk3(mad(step.x, t, pp.x), mad(step.y, t, pp.y), mad(step.z, t, pp.z));
                wq = mk3(mad(wstep.x, t, wp.x), mad(wstep.y, t, wp.y), mad(wstep.z, t, wp.z));
            }
        }
        if constexpr (SURF) {
            dst = make_float4(q.x, q.y, q.z, 1.0f);
            return;
        }
        const float4 s = tex3_rgba<OFF32>(P.vol[0], q);
        const f3 N = normalize3(mk3(s.x, s.y, s.z));  // (zero gradient: NaN -> max(NaN, 0) = 0, ambient only, as LIGHT)
        const f3 sh = shade(N, wq, mk3(P.light_pos[0], P.light_pos[1], P.light_pos[2]), mk3(P.light_dif[0], P.light_dif[1], P.light_dif[2]),
                            mk3(P.light_amb[0], P.light_amb[1], P.light_amb[2]), 2.5f, 0.5f);
        const TfSample c = tf_lookup(P.tf[0], iso);
        blend(mk3(c.rgb.x * sh.x, c.rgb.y * sh.y, c.rgb.z * sh.z), 1.0f, dst);
    });
}

template <bool OFF32, bool SKIP, bool BATCH = false>
__global__ __launch_bounds__(64) void march_iso_kernel(const MarchBatch B)
{
    march_shell<BATCH>(B, [](auto&... a) { iso_packet<OFF32, SKIP>(a...); });
}

// The picking read-back: march_iso_kernel's march with the refined point stored in place of the shading tail
// (iso_packet<.., SURF = true>).  A kernel name of its own: march_iso_kernel keeps exactly the instances it had.
template <bool OFF32, bool SKIP, bool BATCH = false>
__global__ __launch_bounds__(64) void iso_point_kernel(const MarchBatch B)
{
    march_shell<BATCH>(B, [](auto&... a) { iso_packet<OFF32, SKIP, true>(a...); });
}

}  // namespace VR_KNS
