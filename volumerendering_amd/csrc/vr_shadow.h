// vr_shadow.h -- shadows of the lit shader through a light volume (vr_set_shadows, include/vr.h): a coarse grid that holds, per texel,
// the transmittance from the texel's centre toward the light, built once per key (volume, opacity table, light, clip box, divisor,
// scale, arithmetic mode; the ring of vr_api.hip), and LIGHT's march with the diffuse term of every blended sample scaled by one
// trilinear fetch of that grid.  Included by vr_launch.h once per arithmetic mode.
//
// shadow_build_kernel: one texel per lane, one 4 x 4 x 4 block of texels per wavefront (their rays toward the light are nearly
// parallel: they touch the same bricks and cache lines).  Each lane walks from its texel centre toward the light by repeated
// rounded additions q += s, multiplies T by (1 - clamp(scale * opacity)) at every position inside the clip box, and stops when it
// leaves the unit cube, reaches the light or T falls below 2^-10.  SKIP (flavour 23): a position whose base cell lies in a brick
// that LIGHT's distance field marks inert (byte != 0) has opacity exactly 0 -- the field's own guarantee -- so T is unchanged and
// nothing is loaded; the addition still runs, because the positions are defined by it.
//
// march_shadow_kernel: LIGHT's march (vr_kernels.h march_packet: positions, world positions, variable step, jitter, the cut-off
// dst.a < 1, fragment modes 1-4, the blend and the counters), one lane per ray, one 8x8 packet per wavefront (map_pixel), the next
// step's corner loads issued before this step is interpolated.  A blended sample also reads S = the light volume at p (MarchParams::
// vol[1]: x-fastest float plane, bricked = 0, lut = 0, so tex3_a's texel pairs and lerps) and its diffuse term dif * m becomes
// dif * (m * S).  SKIP (flavour 23): a step in an inert brick of LIGHT's distance field (P.brick_dist) loads nothing, and a sample
// whose opacity is exactly 0 (opacity_is_zero) is not shaded and reads no S -- both are the identity blend, as in LIGHT's skipping
// forms (the host enables them only when a zero-opacity sample provably is: finite colour table and light).
#pragma once

namespace VR_KNS {

// BASIC's opacity look-up of density d (tf_fetch + tf_finish's opacity: the same index, weight and lerp; the colour is not loaded)
__device__ __forceinline__ float tf_opacity(const DevTF& tf, float d)
{
    const float xo = mad(d, (float)tf.res_o, -0.5f);
    const float xo0 = floorf(xo);
    const int jo = padded_texel(xo0, tf.res_o);
    const float* po = reinterpret_cast<const float*>(reinterpret_cast<const char*>(tf.opacity) + ((unsigned)jo << 2));
    return lerpf(po[0], po[1], xo - xo0);
}

// P: the LIGHT launch's parameters (vol[0], tf[0], the clip box, light_pos of its frame, with SKIP the distance field) and
// vol[1] = the grid; out = the grid's storage (vol[1].dens), sigma = the opacity scale.
template <bool OFF32, bool SKIP>
__global__ __launch_bounds__(64) void shadow_build_kernel(const MarchParams P, float* out, float sigma)
{
    const int gx = P.vol[1].nx, gy = P.vol[1].ny, gz = P.vol[1].nz;
    const unsigned cbx = ((unsigned)gx + 3u) >> 2, cby = ((unsigned)gy + 3u) >> 2;
    const unsigned b = blockIdx.x, lane = threadIdx.x;
    const int i = (int)((b % cbx) * 4u + (lane & 3u));
    const int j = (int)(((b / cbx) % cby) * 4u + ((lane >> 2) & 3u));
    const int k = (int)((b / cbx / cby) * 4u + (lane >> 4));
    if (i >= gx || j >= gy || k >= gz) return;
    // the light in texture space (setup_ray's world-to-uvw map of the box), the step length, the texel's centre
    const f3 l = mk3(P.light_pos[0] + 0.5f, P.light_pos[1] + 0.5f, 0.5f - 2.0f * P.light_pos[2]);
    const float h = 1.0f / (float)max(max(gx, gy), gz);
    const f3 c = mk3(((float)i + 0.5f) / (float)gx, ((float)j + 0.5f) / (float)gy, ((float)k + 0.5f) / (float)gz);
    const f3 D = mk3(l.x - c.x, l.y - c.y, l.z - c.z);
    const float len = length3s(D);
    const f3 dir = normalize3s(D);
    const f3 s = mk3(dir.x * h, dir.y * h, dir.z * h);
    const float lim = len / h;
    const int K = lim < 65536.0f ? (int)lim : 65536;  // (NaN: 65536)
    const float bx0 = P.bmin[0], by0 = P.bmin[1], bz0 = P.bmin[2];
    const float bx1 = P.bmax[0], by1 = P.bmax[1], bz1 = P.bmax[2];
    float T = 1.0f;
    f3 q = c;
    for (int n = 1; n <= K; ++n) {
        q = mk3(q.x + s.x, q.y + s.y, q.z + s.z);
        if (!(q.x >= 0.0f && q.x <= 1.0f && q.y >= 0.0f && q.y <= 1.0f && q.z >= 0.0f && q.z <= 1.0f)) break;  // (NaN leaves)
        if (!(q.x >= bx0 && q.x <= bx1 && q.y >= by0 && q.y <= by1 && q.z >= bz0 && q.z <= bz1)) continue;
        if constexpr (SKIP) {
            if (dist_at(P, brick_of<OFF32>(P, q)) != 0u) continue;  // inert brick: opacity exactly 0, T unchanged
        }
        const float d = tex3_a<OFF32>(P.vol[0], q);
        float a = sigma * tf_opacity(P.tf[0], d);
        a = a > 1.0f ? 1.0f : a;
        a = a > 0.0f ? a : 0.0f;  // (NaN -> 0)
        T = T * (1.0f - a);
        if (T < 0x1p-10f) break;
    }
    out[((size_t)k * (size_t)gy + (size_t)j) * (size_t)gx + (size_t)i] = T;
}

// One ray: what a lane does for its pixel `slot` (LIGHT's march_packet, shadowed).
template <bool OFF32, bool SKIP>
__device__ __forceinline__ void shadow_packet(const MarchParams& P, const PixelSlot& slot, float4& dst, unsigned& blends, unsigned& covered,
                                              unsigned& fetched)
{
    RayStart r;
    // (covered: every pixel whose ray hits the box, as LIGHT's march_packet)
    covered = with_ray(P, slot, dst, r, [&]() __attribute__((always_inline)) {
        f3 p = r.p, w = r.world0;
        const f3 step = r.step, wstep = world_step(P, r.dir);
        const int n_steps = P.steps_count;
        const f3 lpos = mk3(P.light_pos[0], P.light_pos[1], P.light_pos[2]);
        const f3 dif = mk3(P.light_dif[0], P.light_dif[1], P.light_dif[2]);
        const f3 amb = mk3(P.light_amb[0], P.light_amb[1], P.light_amb[2]);
        unsigned n = 0;

        // step i: corners of p in F (requested one iteration ago) when `have`; R = distance-field byte of p + step (requested one
        // iteration ago)
        Fetch4 F;
        float fx = 0.0f, fy = 0.0f, fz = 0.0f;
        bool have = false;
        unsigned R = 0;
        if (n_steps > 0 && in_box(P, r, 0, p)) {
            have = !SKIP || dist_at(P, brick_of<OFF32>(P, p)) == 0u;
            if (have) fetch_rgba<OFF32>(P.vol[0], p, F, fx, fy, fz);
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
            // this step's sample: its table texels and its light-volume corners are requested before the next step's corners, so that
            // waiting for them leaves those eight loads in flight
            const bool sample = inb && have;
            bool shaded = false;
            v2f zw = v2f{0.0f, 0.0f}, gxy = zw;
            TfFetch tq = {};
            Fetch1 Sq = {};
            float sx = 0.0f, sy = 0.0f, sz = 0.0f;
            if (sample) {
                zw = interp_zw(F, fx, fy, fz);  // (gradient z, density)
                shaded = !SKIP || !opacity_is_zero(P, zw.y);
                if (shaded) {
                    tq = tf_fetch(P.tf[0], zw.y);
                    gxy = interp_xy(F, fx, fy, fz);
                    fetch_a<OFF32>(P.vol[1], p, Sq, sx, sy, sz);
                }
            }
            Fetch4 G;
            float gx = 0.0f, gy = 0.0f, gz = 0.0f;
            __builtin_amdgcn_sched_barrier(0);
            if (next) fetch_rgba<OFF32>(P.vol[0], pn, G, gx, gy, gz);
            __builtin_amdgcn_sched_barrier(0);
            if (inb) {
                ++n;
                if (sample) {
                    ++fetched;
                    if (shaded) {
                        const float S = interp_a(Sq, sx, sy, sz);
                        shade_blend_packed<false, false, true>(lpos, dif, amb, 2.5f, 0.5f, w, zw, gxy, tq, dst, false, f3{0.0f, 0.0f, 0.0f},
                                                               0.0f, S);
                    }
                    if (!(dst.w < 1.0f)) break;  // LIGHT's cut-off: no later iteration can blend
                }
            }
            F = G;
            fx = gx;
            fy = gy;
            fz = gz;
            have = next;
            p = pn;
            w = mk3(w.x + wstep.x, w.y + wstep.y, w.z + wstep.z);
        }
        blends = n;
    });
}

template <bool OFF32, bool SKIP, bool BATCH = false>
__global__ __launch_bounds__(64) void march_shadow_kernel(const MarchBatch B)
{
    march_shell<BATCH>(B, [](auto&... a) { shadow_packet<OFF32, SKIP>(a...); });
}

}  // namespace VR_KNS
