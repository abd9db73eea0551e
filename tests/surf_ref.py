"""float32 numpy restatement of the surface-position output of include/vr.h (vr_set_output(VR_OUTPUT_SURFACE)) in either
arithmetic mode: BASIC's sample positions as proj_ref.march places them (rays from oracle_binding.setup_ray, jitter from
oracle_binding.jitter), the alpha line of FrontToBackBlend accumulated through proj_ref's sampler and opacity look-up, the first
in-box step after whose blend a > tau, the secant refinement on alpha, the depth formula of vr_surface_depth_async and the record of
vr_pick.  The isosurface's surface output is iso_ref.march's refined point.  With fused=True the sampler's and the look-up's
coordinates and lerps, the alpha line a = mad(1 - a, o, a) and the refinement q = mad(step, t, p_{k-1}) are single fused multiply-adds;
the positions, the division t and the depth's matrix products are separately rounded in both modes.  Harness only."""
import numpy as np

import iso_ref as ir
import oracle_binding as ob
import proj_ref as pr
from fma_ref import mad

f32 = np.float32
BASIC, LIGHT, ISO = 0, 1, 11
TAU_BASIC = f32(0.95)                          # BASIC's cut-off dst.a <= 0.95
TAU_LIGHT = f32(np.nextafter(f32(1.0), f32(0.0)))  # 0x1.fffffep-1f: a > tau <=> !(a < 1.0), LIGHT's cut-off


def opacity_lookup(opacity, d, fused=False):
    """BASIC's opacity look-up of densities d (linear, clamp-to-edge): proj_ref.tf_lookup's opacity half."""
    return pr.opacity_lookup(opacity, d, fused)


def march(u, W, H, vec4, opacity, tau, pixels=None, positions=False, fused=False):
    """Surface output of BASIC / LIGHT for `pixels` (px, py) (default: the whole frame, row by row).  Returns a dict: frag (N, 4),
    composited (N,), hit (N,), rayhit (N,) = the ray goes through the box, k (N,) = the hit's step index (-1 without one), first (N,)
    = the hit is the ray's first in-box step, q / pk / pp (N, 3) = the refined point, the hit step's position and the position of the
    step before it (NaN where there is no hit), pixels; with `positions` also positions (steps, N, 3) = every step's p_i (NaN for
    pixels without a ray), which no threshold and no arithmetic mode changes."""
    if pixels is None:
        pixels = np.stack(np.meshgrid(np.arange(W), np.arange(H)), -1).reshape(-1, 2)
    pixels = np.asarray(pixels, dtype=np.int64).reshape(-1, 2)
    dens = np.ascontiguousarray(np.asarray(vec4, dtype=f32)[..., 3])
    opacity = np.asarray(opacity, dtype=f32)
    tau = f32(tau)
    N = len(pixels)
    out = dict(frag=np.zeros((N, 4), f32), composited=np.zeros(N, np.int64), hit=np.zeros(N, bool), rayhit=np.zeros(N, bool),
               k=np.full(N, -1, np.int64), first=np.zeros(N, bool), q=np.full((N, 3), np.nan, f32), pk=np.full((N, 3), np.nan, f32),
               pp=np.full((N, 3), np.nan, f32), pixels=pixels)
    start, end = np.zeros((N, 3), f32), np.zeros((N, 3), f32)
    for i, (px, py) in enumerate(pixels):
        h, s, e, _ = ob.setup_ray(u, W, H, int(px), int(py))
        out["rayhit"][i], start[i], end[i] = h, s, e
    assert u.fragment_mode == 0
    idx = np.nonzero(out["rayhit"])[0]
    if idx.size == 0 or u.steps_count <= 0:
        return out
    M = idx.size
    with np.errstate(all="ignore"):
        diff = end[idx] - start[idx]
        ln = np.sqrt((diff[:, 0] * diff[:, 0] + diff[:, 1] * diff[:, 1]) + diff[:, 2] * diff[:, 2])
        dr = diff * (f32(1.0) / ln)[:, None]
        ss = np.full(M, f32(u.step_size), f32)
        if u.toggles[0] == 1:
            ss = ln / f32(u.steps_count)
        p = start[idx].copy()
        if u.toggles[1] == 1:
            j = np.array([ob.jitter(float(f32(px) + f32(0.5)), float(f32(py) + f32(0.5))) for px, py in pixels[idx]], f32)
            p = p + (dr * ss[:, None]) * j[:, None]
        step = dr * ss[:, None]
    lo = np.array([f32(0.0) + f32(u.clip_x[0]), f32(0.0) + f32(u.clip_y[0]), f32(0.0) + f32(u.clip_z[0])], f32)
    hi = np.array([f32(1.0) - f32(u.clip_x[1]), f32(1.0) - f32(u.clip_y[1]), f32(1.0) - f32(u.clip_z[1])], f32)
    n = np.zeros(M, np.int64)
    a, a_prev = np.zeros(M, f32), np.zeros(M, f32)
    hit, first, prev_inb = np.zeros(M, bool), np.zeros(M, bool), np.zeros(M, bool)
    kk = np.full(M, -1, np.int64)
    pk, pp = np.zeros((M, 3), f32), np.zeros((M, 3), f32)
    if positions:
        out["positions"] = np.full((u.steps_count, N, 3), np.nan, f32)
    for i in range(u.steps_count):
        if positions:
            out["positions"][i, idx] = p
        with np.errstate(all="ignore"):
            run = a <= tau  # (false once a ray has hit, and for a NaN alpha)
            inb = run & np.all((p >= lo) & (p <= hi), axis=1)
            o = opacity_lookup(opacity, pr.sample_a(dens, p, fused), fused)
            new = mad(f32(1.0) - a, o, a, fused)
        n += inb
        a_prev[inb] = a[inb]
        a[inb] = new[inb]
        with np.errstate(all="ignore"):
            now = inb & (a > tau)
        pk[now], kk[now], first[now] = p[now], i, ~prev_inb[now]
        hit |= now
        go = run & ~now
        pp[go], prev_inb[go] = p[go], inb[go]
        with np.errstate(all="ignore"):
            p = p + step
    q = pk.copy()
    with np.errstate(all="ignore"):
        t = (tau - a_prev) / (a - a_prev)
        ok = hit & ~first & (t >= f32(0.0)) & (t <= f32(1.0))
        q[ok] = mad(step[ok], t[ok][:, None], pp[ok], fused)
    frag = np.zeros((M, 4), f32)
    frag[:, 3] = a
    frag[hit, :3] = q[hit]
    h = np.nonzero(hit)[0]
    out["frag"][idx] = frag
    out["composited"][idx] = n
    out["hit"][idx] = hit
    out["k"][idx] = kk
    out["first"][idx] = first
    out["q"][idx[h]], out["pk"][idx[h]] = q[h], pk[h]
    nf = h[~first[h]]
    out["pp"][idx[nf]] = pp[nf]
    return out


def frame(u, W, H, vec4, opacity, tau, fused=False):
    """(frag [H, W, 4], composited, covered = pixels with a hit) of the whole frame."""
    r = march(u, W, H, vec4, opacity, tau, fused=fused)
    return r["frag"].reshape(H, W, 4), int(r["composited"].sum()), int(r["hit"].sum())


def iso_frame(u, W, H, vec4, tf, iso, fused=False):
    """Surface output of ISO: (q, 1) on the hit pixels of iso_ref.march, zeros elsewhere; (frag, composited, covered)."""
    r = ir.march(u, W, H, vec4, tf, iso, fused=fused)
    frag = np.zeros((W * H, 4), f32)
    frag[r["hit"], :3] = r["q"][r["hit"]]
    frag[r["hit"], 3] = f32(1.0)
    return frag.reshape(H, W, 4), int(r["composited"].sum()), int(r["covered"].sum())


def _mat_point(m, x, y, z, w):
    """column-major mat4 * (x, y, z, w), summed left to right (the ray set-up's product); arrays broadcast."""
    m = np.asarray(list(m), f32)
    with np.errstate(all="ignore"):
        return [((m[0 + r] * x + m[4 + r] * y) + m[8 + r] * z) + m[12 + r] * w for r in range(4)]


def world_of(q):
    """The inverse of setup_ray's world-to-uvw map, q (..., 3) float32."""
    q = np.asarray(q, f32)
    return np.stack([q[..., 0] - f32(0.5), q[..., 1] - f32(0.5), (f32(0.5) - q[..., 2]) * f32(0.5)], -1)


def depth(frag, u, tau):
    """vr_surface_depth_async of a surface frame (..., 4): 1.0 where !(.w > tau), else clip.z / clip.w of the point."""
    frag = np.asarray(frag, f32)
    w = world_of(frag[..., :3])
    e = _mat_point(u.view, w[..., 0], w[..., 1], w[..., 2], f32(1.0))
    c = _mat_point(u.proj, e[0], e[1], e[2], e[3])
    with np.errstate(all="ignore"):
        d = (c[2] / c[3]).astype(f32)
        return np.where(frag[..., 3] > f32(tau), d, f32(1.0)).astype(f32)


def pick(variant, u, W, H, vols, tf, tau, x, y, iso=0.5, fused=False):
    """The vr_pick_result of pixel (x, y) as a dict of numpy values.  vols: the uploaded slots (None = empty), tf = (opacity, colour)."""
    if variant == ISO:
        r = ir.march(u, W, H, vols[0], tf, iso, pixels=[(x, y)], fused=fused)
        px = np.zeros(4, f32)
        if r["hit"][0]:
            px[:3], px[3] = r["q"][0], f32(1.0)
    else:
        px = march(u, W, H, vols[0], tf[0], tau, pixels=[(x, y)], fused=fused)["frag"][0]
    out = dict(hit=int(px[3] > f32(tau)), uvw=np.zeros(3, f32), world=np.zeros(3, f32), depth=f32(1.0), alpha=f32(px[3]),
               voxel=np.zeros(3, np.int32), value=np.zeros((3, 4), f32))
    if not out["hit"]:
        return out
    out["uvw"] = px[:3].copy()
    out["world"] = world_of(px[:3])
    out["depth"] = depth(px, u, tau)[()]
    nz, ny, nx = np.asarray(vols[0]).shape[:3]
    n = np.array([nx, ny, nz])
    with np.errstate(all="ignore"):
        f = np.floor(px[:3] * n.astype(f32))
    vox = np.clip(np.where(np.isnan(f), 0, f), 0, n - 1).astype(np.int32)
    out["voxel"] = vox
    for i, v in enumerate(vols):
        if v is not None and np.asarray(v).shape[:3] == (nz, ny, nx):
            out["value"][i] = np.asarray(v, f32)[vox[2], vox[1], vox[0]]
    return out
