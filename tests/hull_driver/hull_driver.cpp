// hull_driver -- csrc/vr_hull.h compiled for the CPU (tests/test_hull.py): the plane bounds the host derives, the steps a ray is
// given, and what they are checked against -- the box function the hull replaced, kept here as the reference of the three axes,
// and a walk over the ray's positions (the kernels' rounded additions and brick_of) against a brick set.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <random>

#include "vr_hull.h"

using namespace vr;

namespace {

// The function steps_near_hull replaced, as it stood (the device reciprocal read as VR_HULL_RCP, as the header reads it here).
void steps_near_box(const float pp[3], const float ss[3], const float* box, int n_steps, int& k0, int& k1)
{
    const float drift = (float)n_steps * 4.8e-7f;
    float t0 = 0.0f, t1 = (float)n_steps;
    bool miss = false;
    for (int a = 0; a < 3; ++a) {
        const float lo = box[a] - drift, hi = box[3 + a] + drift;
        if (ss[a] == 0.0f) {
            miss = miss || pp[a] < lo || pp[a] > hi;
        } else {
            const float inv = VR_HULL_RCP(ss[a]);
            const float ta = (lo - pp[a]) * inv, tb = (hi - pp[a]) * inv;
            t0 = fmaxf(t0, fminf(ta, tb));
            t1 = fminf(t1, fmaxf(ta, tb));
        }
    }
    miss = miss || t0 > t1 + 4.0f;
    k0 = miss ? 0x7fffffff : std::max((int)fminf(t0 * 0.999f, 2.0e9f) - 2, 0);
    k1 = miss ? -1 : (int)fminf(t1 * 1.001f + 3.0f, 2.0e9f);
}

HullPlanes planes_of(const float* v)
{
    HullPlanes h;
    std::memcpy(h.lo, v, sizeof h.lo);
    std::memcpy(h.hi, v + kHullDirs, sizeof h.hi);
    return h;
}

// brick_of (vr_kernels.h): clamp(floor(p * bs - half), 0, bn - 1) per axis, the product and the sum rounded separately or fused
int brick_axis(float p, float bs, int bn, float half, bool fused)
{
    const float q = fused ? fmaf(p, bs, -half) : p * bs - half;
    if (!(q > 0.0f)) return 0;  // (a NaN comes out as 0)
    const float top = (float)(bn - 1);
    return (int)floorf(q < top ? q : top);
}

}  // namespace

extern "C" {

int hd_dirs(int* out)
{
    for (int d = 0; d < kHullDirs; ++d)
        for (int a = 0; a < 3; ++a) out[3 * d + a] = kHullDir[d][a];
    return kHullDirs;
}

// kind 0: from the integer planes; 1: unbounded; 2: inverted.  out = lo[13], hi[13]
void hd_bounds(int kind, const int* lo, const int* hi, const float* bs, float half, float* out)
{
    const HullPlanes h = kind == 1 ? hull_unbounded() : (kind == 2 ? hull_inverted() : hull_bounds(lo, hi, bs, half));
    std::memcpy(out, h.lo, sizeof h.lo);
    std::memcpy(out + kHullDirs, h.hi, sizeof h.hi);
}

void hd_steps(const float* p, const float* s, const float* bs, const float* planes, int n_steps, int axes_only, int* k)
{
    const HullPlanes h = planes_of(planes);
    steps_near_hull(p, s, bs, h, n_steps, k[0], k[1], [&](bool open) { return open && !axes_only; });
}

void hd_steps_box(const float* p, const float* s, const float* box, int n_steps, int* k) { steps_near_box(p, s, box, n_steps, k[0], k[1]); }

// Random sweep of the three axes against the function they replaced: positions, steps (zeros, tiny, huge, NaN, infinities), boxes
// (ordinary, inverted, unbounded, NaN) and counts.  Returns the number of cases whose k0 / k1 differ; *cases = how many had a step
// component that is zero, a NaN, a miss.
int hd_axes_sweep(unsigned seed, int n, int* cases)
{
    std::mt19937 g(seed);
    std::uniform_real_distribution<float> U(0.0f, 1.0f);
    auto pick = [&](int m) { return (int)(g() % (unsigned)m); };
    auto value = [&](float lo, float hi) { return lo + (hi - lo) * U(g); };
    auto odd = [&](float v) {
        switch (pick(24)) {
        case 0: return 0.0f;
        case 1: return -0.0f;
        case 2: return NAN;
        case 3: return INFINITY;
        case 4: return -INFINITY;
        case 5: return v * 1.0e-30f;
        case 6: return v * 1.0e-42f;  // (subnormal)
        case 7: return v * 1.0e30f;
        default: return v;
        }
    };
    int bad = 0;
    cases[0] = cases[1] = cases[2] = 0;
    const float bs[3] = {24.0f, 16.0f, 20.0f};
    for (int i = 0; i < n; ++i) {
        float p[3], s[3];
        HullPlanes h = hull_unbounded();
        const int n_steps = pick(8) == 0 ? 1 + pick(4000) : (pick(2) ? 886 : 4000);
        const float len = pick(4) == 0 ? 1.0e-6f : 2.0f / (float)n_steps;
        const int kind = pick(8);
        for (int a = 0; a < 3; ++a) {
            p[a] = odd(value(-0.5f, 1.5f));
            s[a] = odd(value(-len, len));
            float lo = value(-0.2f, 1.0f), hi = lo + value(0.0f, 0.8f);
            if (kind == 0) { lo = 3.0e38f; hi = -3.0e38f; }
            if (kind == 1) { lo = -3.0e38f; hi = 3.0e38f; }
            if (kind == 2) { lo = odd(lo); hi = odd(hi); }
            h.lo[a] = lo;
            h.hi[a] = hi;
        }
        const float box[6] = {h.lo[0], h.lo[1], h.lo[2], h.hi[0], h.hi[1], h.hi[2]};
        int a0, a1, b0, b1;
        steps_near_box(p, s, box, n_steps, a0, a1);
        steps_near_hull(p, s, bs, h, n_steps, b0, b1, [](bool) { return false; });
        bad += a0 != b0 || a1 != b1;
        cases[0] += s[0] == 0.0f || s[1] == 0.0f || s[2] == 0.0f;
        cases[1] += std::isnan(p[0] + p[1] + p[2] + s[0] + s[1] + s[2]);
        cases[2] += a1 < 0;
    }
    return bad;
}

// n_rays rays against a brick set (set[(z * bn[1] + y) * bn[0] + x] != 0: the brick is in it): the positions p_k = fl(p_{k-1} + s),
// k < n_steps[r], every one inside [0, 1]^3 (IsInSampleCoords without clipping: the only positions a march samples) whose brick is
// in the set must have k0 <= k <= k1.  Returns how many do not; k[2 r], k[2 r + 1] = the ray's k0, k1; in_set[r] = its steps in the
// set.  fused: brick_of's arithmetic.
long long hd_walk(const unsigned char* set, const int* bn, const float* bs, float half, const float* planes, int n_rays, const float* p,
                  const float* s, const int* n_steps, int fused, int* k, int* in_set)
{
    const HullPlanes h = planes_of(planes);
    long long bad = 0;
    for (int r = 0; r < n_rays; ++r) {
        const float* p0 = p + 3 * r;
        const float* st = s + 3 * r;
        int k0, k1;
        steps_near_hull(p0, st, bs, h, n_steps[r], k0, k1, [](bool open) { return open; });
        k[2 * r] = k0;
        k[2 * r + 1] = k1;
        float q[3] = {p0[0], p0[1], p0[2]};
        int hits = 0;
        for (int i = 0; i < n_steps[r]; ++i) {
            if (q[0] >= 0.0f && q[0] <= 1.0f && q[1] >= 0.0f && q[1] <= 1.0f && q[2] >= 0.0f && q[2] <= 1.0f) {
                const int bx = brick_axis(q[0], bs[0], bn[0], half, fused != 0), by = brick_axis(q[1], bs[1], bn[1], half, fused != 0),
                          bz = brick_axis(q[2], bs[2], bn[2], half, fused != 0);
                if (set[((size_t)bz * bn[1] + by) * bn[0] + bx]) {
                    ++hits;
                    bad += i < k0 || i > k1;
                }
            }
            for (int a = 0; a < 3; ++a) {
                volatile float t = q[a] + st[a];  // (a rounded f32 addition whatever the compiler keeps in wider registers)
                q[a] = t;
            }
        }
        in_set[r] = hits;
    }
    return bad;
}

}  // extern "C"
