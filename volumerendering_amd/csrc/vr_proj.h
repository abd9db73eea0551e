// vr_proj.h -- intensity projections of volume slot 0 (VR_VARIANT_MIP / MINIP / AVERAGE, include/vr.h): the BASIC shader's march
// (same start, direction, steps, step size, variable step, jitter and rounded additions p += step), but instead of compositing, the
// samples inside IsInSampleCoords are reduced to one value -- their maximum, their minimum or their mean -- which then goes through
// TF slot 0 and one FrontToBackBlend onto dst = 0.  One lane per ray, one 8x8 packet per wavefront (map_pixel: launch order, packed
// tiles, the (frame, packet) items of batched launches).  Included by vr_launch.h once per arithmetic mode.
//
// Exact skipping (SKIP): a step whose base cell lies in a brick (brick_of) that cannot change the running result loads nothing.
//   MIP:   brick max <= m            MinIP: brick min >= m            AIP: every voxel the brick can touch is +-0
// The brick records are (min .a, max .a) over the (c+1)^3 voxels a brick of c^3 base cells can touch (brick_range_kernel); a record
// holding a NaN, an infinity or a magnitude above 2^125 is (NaN, NaN), which fails every comparison: never skipped.
// Why a brick's range bounds every sample in it: a trilinear sample is seven lerps r = a + (b - a) * t, t = the cell fraction.
//   t is in [0, 1 - 2^-24] unless the texel pair is clamped at a face (then a == b and r = a + 0 * t = a exactly): x - floor(x) is exact
//   for x >= 0 (Sterbenz), and a cell coordinate in [-1, 0) -- where x + 1 may round up to 1 -- clamps both texels to 0.
//   Let a <= b (b < a is the same with both negated), |a|, |b| <= 2^125 so that d = fl(b - a) is finite, d = b - a + e, |e| <= ulp(d) / 2.
//   r >= a: d >= 0, so every rounded step of a + d * t is >= a (rounding is monotone).
//   r <= b, separate rounding: d * t <= d - d * 2^-24 lies below the midpoint between d and its lower neighbour whenever d is normal,
//     so q = fl(d * t) <= d - ulp(d) / 2 and a + q <= b + e - ulp(d) / 2 <= b, hence fl(a + q) <= b.  (d subnormal: b - a is exact,
//     e = 0, q <= d, a + q <= b.)
//   r <= b, fused: a + d * t <= b + e - d * 2^-24 <= b since |e| <= ulp(d) / 2 <= d * 2^-24 (d normal; subnormal: e = 0).
//   The corner values of every lerp level lie in [min, max] of the eight voxels, so the sample does: no margin is needed.  (Checked by
//   an adversarial search in both modes: tests/test_projection.py.)
// NaN samples: MIP and MinIP ignore them (`d > m` / `d < m` is false), AIP propagates them -- the NaN voxel's brick is never skipped.
// AIP: s starts at +0 and x + (-x) rounds to +0, so s is never -0 and adding a +-0 sample leaves it bit-identical.
// Early exit (SKIP only): once MIP's m >= the volume's maximum (MinIP: m <= its minimum) no later sample can change m; the ray keeps
// its rounded additions and its in-box test to count n, and loads nothing more.
// The loop issues the corner loads of the next step before it interpolates this one, and looks each brick record up two steps
// ahead, so that waiting for a record never waits for the corners still in flight (loads complete in order).
#pragma once

namespace VR_KNS {

enum ProjMode : int { kProjMax = 0, kProjMin = 1, kProjAvg = 2 };

// record of the brick of p (the base cell's brick, brick_of) for the skipping test below
__device__ __forceinline__ float2 proj_record(const MarchParams& P, f3 p) { return brick_record(P, brick_of<true>(P, p)); }

template <int MODE>
__device__ __forceinline__ bool proj_inert(float2 rec, float m)
{
    if constexpr (MODE == kProjMax) return rec.y <= m;
    else if constexpr (MODE == kProjMin) return rec.x >= m;
    else return rec.x == 0.0f && rec.y == 0.0f;  // (+-0 compare equal; the NaN record fails)
}

template <int MODE>
__device__ __forceinline__ void proj_update(float& m, float d)
{
    if constexpr (MODE == kProjMax) {
        if (d > m) m = d;
    } else if constexpr (MODE == kProjMin) {
        if (d < m) m = d;
    } else {
        m = m + d;
    }
}

// One ray: what a lane does for its pixel `slot`.  vrange = (min, max) of the whole volume (NaN if flagged), SKIP only.
template <int MODE, bool OFF32, bool SKIP>
__device__ __forceinline__ void proj_packet(const MarchParams& P, const float2* __restrict__ vrange, const PixelSlot& slot, float4& dst,
                                            unsigned& samples, unsigned& covered, unsigned& fetched)
{
    RayStart r;
    with_ray(P, slot, dst, r, [&]() __attribute__((always_inline)) {
        f3 p = r.p;
        const f3 step = r.step;
        const int n_steps = P.steps_count;
        float m = MODE == kProjMax ? -INFINITY : (MODE == kProjMin ? INFINITY : 0.0f);
        float lim = 0.0f;  // early exit: MIP m >= lim, MinIP m <= lim (NaN: never)
        if constexpr (SKIP && MODE != kProjAvg) lim = MODE == kProjMax ? vrange->y : vrange->x;
        bool done = false;
        unsigned n = 0;

        // step i: corners of p in F (requested one iteration ago) when `have`; R = record of p + step (requested one iteration ago)
        Fetch1 F;
        float fx = 0.0f, fy = 0.0f, fz = 0.0f;
        bool have = false;
        float2 R = make_float2(0.0f, 0.0f);
        if (n_steps > 0 && in_box(P, r, 0, p)) {
            have = !SKIP || !proj_inert<MODE>(proj_record(P, p), m);
            if (have) fetch_a<OFF32>(P.vol[0], p, F, fx, fy, fz);
        }
        if constexpr (SKIP) R = proj_record(P, mk3(p.x + step.x, p.y + step.y, p.z + step.z));
        for (int i = 0; i < n_steps; ++i) {
            const bool inb = in_box(P, r, i, p);
            if (!inb && gone(P, step, p)) break;
            const f3 pn = mk3(p.x + step.x, p.y + step.y, p.z + step.z);
            // the next step: loaded unless it is outside the box or its brick cannot change m as m stands now (m only ever moves
            // towards the side that makes more bricks inert, so the test stays true when it is applied one step early)
            bool next = i + 1 < n_steps && !done && in_box(P, r, i + 1, pn);
            if constexpr (SKIP) {
                next = next && !proj_inert<MODE>(R, m);
                R = proj_record(P, mk3(pn.x + step.x, pn.y + step.y, pn.z + step.z));  // (issued before the corners below)
            }
            Fetch1 G;
            float gx = 0.0f, gy = 0.0f, gz = 0.0f;
            __builtin_amdgcn_sched_barrier(0);
            if (next) fetch_a<OFF32>(P.vol[0], pn, G, gx, gy, gz);
            __builtin_amdgcn_sched_barrier(0);
            if (inb) {
                ++n;
                if (have) {
                    proj_update<MODE>(m, interp_a(F, fx, fy, fz));
                    ++fetched;
                    if constexpr (SKIP && MODE == kProjMax) done = m >= lim;
                    if constexpr (SKIP && MODE == kProjMin) done = m <= lim;
                }
            }
            F = G;
            fx = gx;
            fy = gy;
            fz = gz;
            have = next;
            p = pn;
        }
        samples = n;
        if (n == 0) return;
        covered = 1;
        float v = m;
        if constexpr (MODE == kProjAvg) v = m / (float)n;
        const TfSample t = tf_lookup(P.tf[0], v);
        blend(t.rgb, t.opacity, dst);
    });
}

template <int MODE, bool OFF32, bool SKIP, bool BATCH = false>
__global__ __launch_bounds__(64) void march_proj_kernel(const MarchBatch B, const float2* __restrict__ vrange)
{
    march_shell<BATCH>(B, [&](const MarchParams& P, auto&... a) { proj_packet<MODE, OFF32, SKIP>(P, vrange, a...); });
}

}  // namespace VR_KNS
