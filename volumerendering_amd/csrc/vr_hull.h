// vr_hull.h -- the convex proxy of the active bricks a skipping launch prunes its rays with: 13 pairs of planes, the
// 3 axes, the 6 face diagonals and the 4 body diagonals of the brick grid, around the active bricks of the distance field.
// Plain C++ with no HIP type: vr_device.h includes it for MarchParams' plane pairs, vr_ctx.h turns a build's integer planes into bounds
// (hull_bounds), the skipping march kernels ask steps_near_hull which steps of a ray can lie in an active brick, and tests/hull_driver
// compiles it with g++ to sweep that answer on the CPU.  The device's reciprocal comes in through VR_HULL_RCP.
#pragma once
#include <math.h>

#ifndef VR_HULL_FN
#define VR_HULL_FN inline
#endif
#ifndef VR_HULL_RCP
#define VR_HULL_RCP(x) (1.0f / (x))  // (the kernels: v_rcp_f32, 1 ulp -- the slack below is a thousand times that)
#endif

namespace vr {

constexpr int kHullAxes = 3;    // the first three directions are the axes: their pair is the box of the active bricks
constexpr int kHullDirs = 13;
constexpr int kHullDiag = kHullDirs - kHullAxes;  // the ten diagonals
constexpr int kHullDir[kHullDirs][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1},  {1, 1, 0}, {1, -1, 0},  {1, 0, 1}, {1, 0, -1},
                                        {0, 1, 1}, {0, 1, -1}, {1, 1, 1}, {1, 1, -1}, {1, -1, 1}, {1, -1, -1}};
// n . b of a brick b, biased so that it is positive whatever the direction (a grid has at most 2^14 bricks per axis): the device
// reduction keeps "all zeros is empty" for the diagonals as it does for the axes
constexpr int kHullBias = 1 << 16;

// The plane pairs a launch reads (MarchParams::abox and ::hull_lo / ::hull_hi; wave-uniform scalar loads, once per packet).
//   d < 3:  lo[d] <= p_d <= hi[d] in uvw -- the box of the active bricks with one brick of margin, as it always was
//   d >= 3: lo[d] <= g . p <= hi[d] with g = n o bs (bricks per unit of uvw, signed by the direction; exact in f32)
// outside of which no position lies in an active brick.
struct HullPlanes {
    float lo[kHullDirs], hi[kHullDirs];
};

VR_HULL_FN HullPlanes hull_unbounded()
{
    HullPlanes h;
    for (int d = 0; d < kHullDirs; ++d) {
        h.lo[d] = -3.0e38f;
        h.hi[d] = 3.0e38f;
    }
    return h;
}
// (no active brick: every pair inverted.  steps_near_hull reports a miss for it only where a ray does not move along a direction;
// every other ray counts all its steps as near and skips by the field, which says inert everywhere)
VR_HULL_FN HullPlanes hull_inverted()
{
    HullPlanes h;
    for (int d = 0; d < kHullDirs; ++d) {
        h.lo[d] = 3.0e38f;
        h.hi[d] = -3.0e38f;
    }
    return h;
}

VR_HULL_FN float hull_round_down(double v)
{
    float f = (float)v;
    return (double)f > v ? nextafterf(f, -INFINITY) : f;
}
VR_HULL_FN float hull_round_up(double v)
{
    float f = (float)v;
    return (double)f < v ? nextafterf(f, INFINITY) : f;
}

// The bounds of the active bricks whose n . b spans [ilo[d], ihi[d]] (brick coordinates; bs = bricks per unit of uvw, half = kBrickHalf).
// A position p lies in brick b when q = p o bs - half has b_a <= q_a < b_a + 1, the first and the last brick of an axis holding what
// lies beyond them as well (less than a brick for a position inside the volume): n . q of a position in an active brick lies in
// [lo_n - #(n_a < 0), hi_n + #(n_a > 0)], and one brick per participating axis comes on top as margin.  The axes keep the box's own
// expression (round to nearest: the margin is a whole brick); the diagonals bound g . p = n . q + half * sum(n_a), rounded outward.
VR_HULL_FN HullPlanes hull_bounds(const int ilo[kHullDirs], const int ihi[kHullDirs], const float bs[3], float half)
{
    HullPlanes h;
    for (int a = 0; a < kHullAxes; ++a) {
        h.lo[a] = (float)(((double)ilo[a] - 1.0 + (double)half) / (double)bs[a]);
        h.hi[a] = (float)(((double)ihi[a] + 2.0 + (double)half) / (double)bs[a]);
    }
    for (int d = kHullAxes; d < kHullDirs; ++d) {
        int neg = 0, pos = 0, sum = 0;
        for (int a = 0; a < 3; ++a) {
            neg += kHullDir[d][a] < 0;
            pos += kHullDir[d][a] > 0;
            sum += kHullDir[d][a];
        }
        h.lo[d] = hull_round_down((double)ilo[d] - (double)neg - (double)(neg + pos) + (double)half * (double)sum);
        h.hi[d] = hull_round_up((double)ihi[d] + (double)pos + (double)(neg + pos) + (double)half * (double)sum);
    }
    return h;
}

// Steps [t0, t1] of a ray (as reals) outside of which its positions certainly lie outside the pairs looked at so far; miss: it
// lies outside one of them at every step.
struct HullSpan {
    float t0, t1;
    bool miss;
};

// One pair: positions whose coordinate along the direction is o + k s at step k (as reals), against [lo, hi].  A ray that does not
// move along the direction is only ever in or out.  (fminf / fmaxf drop a NaN operand: a NaN excludes nothing.)
VR_HULL_FN void hull_slab(float o, float s, float lo, float hi, HullSpan& r)
{
    if (s == 0.0f) {
        r.miss = r.miss || o < lo || o > hi;
    } else {
        const float inv = VR_HULL_RCP(s);
        const float ta = (lo - o) * inv, tb = (hi - o) * inv;
        r.t0 = fmaxf(r.t0, fminf(ta, tb));
        r.t1 = fminf(r.t1, fmaxf(ta, tb));
    }
}

// The three axes: the box.  The pairs carry a whole brick of margin, far above what the rounded additions of n_steps steps can drift
// -- 2^-23 per step, allowed for on top -- and what the quotients' evaluation in f32 can be off by (hull_steps' slack).
VR_HULL_FN HullSpan hull_axes(const float p[3], const float s[3], const float lo[kHullAxes], const float hi[kHullAxes], int n_steps)
{
    const float drift = (float)n_steps * 4.8e-7f;
    HullSpan r = {0.0f, (float)n_steps, false};
    for (int a = 0; a < kHullAxes; ++a) hull_slab(p[a], s[a], lo[a] - drift, hi[a] + drift, r);
    return r;
}
VR_HULL_FN bool hull_rejected(const HullSpan& r) { return r.miss || r.t0 > r.t1 + 4.0f; }

// The ten diagonals, in brick units: o = g . p, s = g . step; the drift allowance carried through the direction.  (The sums' own
// rounding -- a few ulps of 3 bs, a hundredth of a brick for the largest grid -- disappears in the margin of two bricks and more.)
// (dlo / dhi: the pairs of directions 3 .. 12)
VR_HULL_FN void hull_diagonals(const float p[3], const float s[3], const float bs[3], const float dlo[kHullDiag], const float dhi[kHullDiag],
                               int n_steps, HullSpan& r)
{
    const float drift = (float)n_steps * 4.8e-7f;
    const float u[3] = {p[0] * bs[0], p[1] * bs[1], p[2] * bs[2]}, v[3] = {s[0] * bs[0], s[1] * bs[1], s[2] * bs[2]};
    for (int d = kHullAxes; d < kHullDirs; ++d) {
        float o = 0.0f, sd = 0.0f, w = 0.0f;
        bool first = true;
        for (int a = 0; a < 3; ++a) {
            const int n = kHullDir[d][a];
            if (n == 0) continue;
            // (the first participating axis has n = +1 in every direction)
            o = first ? u[a] : (n > 0 ? o + u[a] : o - u[a]);
            sd = first ? v[a] : (n > 0 ? sd + v[a] : sd - v[a]);
            w = first ? bs[a] : w + bs[a];
            first = false;
        }
        const float df = drift * w;
        hull_slab(o, sd, dlo[d - kHullAxes] - df, dhi[d - kHullAxes] + df, r);
    }
}

// Steps [k0, k1] outside of which the ray's positions certainly lie in no active brick: the span 0.1 % + 2 / + 3 steps wider (the
// quotients' own evaluation in f32).  A ray that misses: k0 = INT_MAX, k1 = -1.
VR_HULL_FN void hull_steps(const HullSpan& r, int& k0, int& k1)
{
    const bool miss = hull_rejected(r);
    const int a = (int)fminf(r.t0 * 0.999f, 2.0e9f) - 2;
    k0 = miss ? 0x7fffffff : (a > 0 ? a : 0);
    k1 = miss ? -1 : (int)fminf(r.t1 * 1.001f + 3.0f, 2.0e9f);
}

// Steps [k0, k1] of the ray p + k step (positions formed by rounded additions, n_steps of them at most) outside of which no position
// lies in an active brick.  NaN anywhere -> no step is excluded.  `more`: whether the diagonals are looked at for a ray the box has
// not rejected (the kernels: a wave-uniform vote, so that a packet outside the box pays for the three axes alone).
// (lo / hi: the three axes' pairs, dlo / dhi the ten diagonals' -- HullPlanes' arrays, or where a launch keeps them)
template <class More>
VR_HULL_FN void steps_near_hull(const float p[3], const float s[3], const float bs[3], const float lo[kHullAxes], const float hi[kHullAxes],
                                const float dlo[kHullDiag], const float dhi[kHullDiag], int n_steps, int& k0, int& k1, More more)
{
    HullSpan r = hull_axes(p, s, lo, hi, n_steps);
    if (more(!hull_rejected(r))) hull_diagonals(p, s, bs, dlo, dhi, n_steps, r);
    hull_steps(r, k0, k1);
}
template <class More>
VR_HULL_FN void steps_near_hull(const float p[3], const float s[3], const float bs[3], const HullPlanes& h, int n_steps, int& k0, int& k1, More more)
{
    steps_near_hull(p, s, bs, h.lo, h.hi, h.lo + kHullAxes, h.hi + kHullAxes, n_steps, k0, k1, more);
}

}  // namespace vr
