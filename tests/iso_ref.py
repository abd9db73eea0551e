"""float32 numpy restatement of the shaded isosurface of include/vr.h (VR_VARIANT_ISO) in either arithmetic mode: BASIC's
sample positions as proj_ref.march places them (rays from oracle_binding.setup_ray, jitter from oracle_binding.jitter), LIGHT's
world position beside them, the first in-box sample at or above the level, the secant refinement, and the shading in the oracle's
operation order (normalize3 = v * (1 / sqrt(dot)), BlinnPhong, the texel pairs and lerps of the samplers, FrontToBackBlend).
With fused=True the per-sample expressions of the shape a * b + c are single fused multiply-adds (fma_ref.fma32), as the header's
VR_ARITH_FUSED and the oracle's fused LIGHT have them: the samplers' coordinates and lerps, dot3 = mad(z, z', mad(y, y', x * x')) and
with it the sum of squares under normalize3, the shading sum mad(dif * m, kD, amb * kA), the blend, and the refinement's
q = mad(step, t, p_{k-1}), w_q = mad(wstep, t, w_{k-1}).  Placement -- direction, step, wstep, p += step, w += wstep -- and the
division t are separately rounded in both modes.  Harness only."""
import numpy as np

from fma_ref import mad

import oracle_binding as ob
import proj_ref as pr

f32 = np.float32
ISO = 11


def sample_rgba(vec4, p, fused=False):
    """textureSample(vol, linear, p) for points p (N, 3): all four channels, the texel pairs and lerp order of proj_ref.sample_a."""
    return pr.sample(vec4, p, fused)


def dot3(a, b, fused=False):
    if fused:
        with np.errstate(all="ignore"):
            return mad(a[:, 2], b[:, 2], mad(a[:, 1], b[:, 1], a[:, 0] * b[:, 0], True), True)
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def normalize3(a, fused=False):
    with np.errstate(all="ignore"):
        inv = f32(1.0) / np.sqrt(dot3(a, a, fused))
        return a * inv[:, None]


def shade(N, w, lpos, dif, amb, kD, kA, fused=False, S=None):
    """light.diffuse * max(dot(N, L), 0) * kD + light.ambient * kA, L = normalize(lightPos - w) (NaN -> 0); with a shadow term S the
    diffuse factor is dif * (m * S), m * S rounded first in both modes."""
    with np.errstate(all="ignore"):
        L = normalize3(lpos[None, :] - w, fused)
        d = dot3(N, L, fused)
        m = np.where(d > f32(0.0), d, f32(0.0)).astype(f32)
        if S is not None:
            m = (m * S).astype(f32)
        return mad(dif[None, :] * m[:, None], f32(kD), amb[None, :] * f32(kA), fused)


def march(u, W, H, vec4, tf, iso, pixels=None, fused=False):
    """ISO of `pixels` (px, py) (default: the whole frame, row by row).  Returns a dict: frag (N, 4), composited (N,), covered (N,),
    fetched_all (N,) = what the form without skipping fetches (= composited), hit (N,), q / pk (N, 3) = the refined / unrefined
    hit positions (NaN where no hit), first (N,) = the hit is the ray's first in-box step, t (N,) = the refinement's quotient (NaN
    where there is none: no hit, or a hit on the first in-box step), pixels."""
    if pixels is None:
        pixels = np.stack(np.meshgrid(np.arange(W), np.arange(H)), -1).reshape(-1, 2)
    pixels = np.asarray(pixels, dtype=np.int64).reshape(-1, 2)
    vec4 = np.ascontiguousarray(np.asarray(vec4, dtype=f32))
    dens = np.ascontiguousarray(vec4[..., 3])
    opacity, color = (np.asarray(t, dtype=f32) for t in tf)
    iso = f32(iso)
    N = len(pixels)
    out = dict(frag=np.zeros((N, 4), f32), composited=np.zeros(N, np.int64), covered=np.zeros(N, bool), hit=np.zeros(N, bool),
               q=np.full((N, 3), np.nan, f32), pk=np.full((N, 3), np.nan, f32), first=np.zeros(N, bool), t=np.full(N, np.nan, f32),
               pixels=pixels)
    start, end, world0 = (np.zeros((N, 3), f32) for _ in range(3))
    rayhit = np.zeros(N, bool)
    for k, (px, py) in enumerate(pixels):
        h, s, e, w = ob.setup_ray(u, W, H, int(px), int(py))
        rayhit[k], start[k], end[k], world0[k] = h, s, e, w
    assert u.fragment_mode == 0
    idx = np.nonzero(rayhit)[0]
    out["fetched_all"] = out["composited"]
    if idx.size == 0 or u.steps_count <= 0:
        return out
    M = idx.size
    with np.errstate(all="ignore"):
        diff = end[idx] - start[idx]
        ln = np.sqrt((diff[:, 0] * diff[:, 0] + diff[:, 1] * diff[:, 1]) + diff[:, 2] * diff[:, 2])
        dr = diff * (f32(1.0) / ln)[:, None]
        ss = np.full(M, f32(u.step_size), f32)
        wstep = np.stack([dr[:, 0] * (ss * f32(1.0)), dr[:, 1] * (ss * f32(1.0)), dr[:, 2] * (ss * f32(0.5))], 1)
        wstep[:, 2] = wstep[:, 2] * f32(-1.0)
        if u.toggles[0] == 1:
            ss = ln / f32(u.steps_count)
        p = start[idx].copy()
        if u.toggles[1] == 1:
            j = np.array([ob.jitter(float(f32(px) + f32(0.5)), float(f32(py) + f32(0.5))) for px, py in pixels[idx]], f32)
            p = p + (dr * ss[:, None]) * j[:, None]
        step = dr * ss[:, None]
    w = world0[idx].copy()
    lo = np.array([f32(0.0) + f32(u.clip_x[0]), f32(0.0) + f32(u.clip_y[0]), f32(0.0) + f32(u.clip_z[0])], f32)
    hi = np.array([f32(1.0) - f32(u.clip_x[1]), f32(1.0) - f32(u.clip_y[1]), f32(1.0) - f32(u.clip_z[1])], f32)
    n = np.zeros(M, np.int64)
    hit = np.zeros(M, bool)
    pk, wk, pp, wp = (np.zeros((M, 3), f32) for _ in range(4))
    dk, dprev = np.zeros(M, f32), np.zeros(M, f32)
    prev_inb, hit_prev_inb = np.zeros(M, bool), np.zeros(M, bool)
    for _ in range(u.steps_count):
        alive = ~hit
        inb = alive & np.all((p >= lo) & (p <= hi), axis=1)
        d = pr.sample_a(dens, p, fused)
        n += inb
        now = inb & (d >= iso)
        pk[now], wk[now], dk[now] = p[now], w[now], d[now]
        hit_prev_inb[now] = prev_inb[now]
        hit |= now
        go = alive & ~now
        pp[go], wp[go], dprev[go], prev_inb[go] = p[go], w[go], d[go], inb[go]
        with np.errstate(all="ignore"):
            p = p + step
            w = w + wstep
    q, wq = pk.copy(), wk.copy()
    with np.errstate(all="ignore"):
        t = (iso - dprev) / (dk - dprev)
        ok = hit & hit_prev_inb & (t >= f32(0.0)) & (t <= f32(1.0))
        q[ok] = mad(step[ok], t[ok][:, None], pp[ok], fused)
        wq[ok] = mad(wstep[ok], t[ok][:, None], wp[ok], fused)
    h = np.nonzero(hit)[0]
    frag = np.zeros((M, 4), f32)
    if h.size:
        s = sample_rgba(vec4, q[h], fused)
        Nn = normalize3(np.ascontiguousarray(s[:, :3]), fused)
        lpos, dif, amb = (np.asarray(a[:3], f32) for a in (u.light_pos, u.light_diffuse, u.light_ambient))
        sh = shade(Nn, wq[h], lpos, dif, amb, 2.5, 0.5, fused)
        _, c = pr.tf_lookup(opacity, color, np.array([iso], f32), fused)
        with np.errstate(all="ignore"):
            rgb = c * sh
            dst = np.zeros((h.size, 4), f32)
            pr._blend(rgb, np.ones(h.size, f32), dst, np.ones(h.size, bool), fused)
        frag[h] = dst
    out["frag"][idx] = frag
    out["composited"][idx] = n
    out["fetched_all"] = out["composited"]
    out["covered"][idx] = hit
    out["hit"][idx] = hit
    out["q"][idx[h]] = q[h]
    out["pk"][idx[h]] = pk[h]
    out["first"][idx[h]] = ~hit_prev_inb[h]
    later = h[hit_prev_inb[h]]
    out["t"][idx[later]] = t[later]
    return out


def frame(u, W, H, vec4, tf, iso, fused=False):
    """(frag [H, W, 4], composited, covered) of the whole frame."""
    r = march(u, W, H, vec4, tf, iso, fused=fused)
    return r["frag"].reshape(H, W, 4), int(r["composited"].sum()), int(r["covered"].sum())
