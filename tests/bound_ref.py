"""float32 numpy restatement of the per-pixel ray bounds of include/vr.h (vr_set_ray_bounds) in either arithmetic mode: BASIC's
and LIGHT's march as proj_ref.march / shadow_ref.march restate them (rays from oracle_binding.setup_ray, jitter from
oracle_binding.jitter, proj_ref's and iso_ref's samplers, look-ups and blend), with the one exception of the definition: an in-box step
at p counts iff S_near <= sigma(p) < S_far, S = sigma of the bound's depth unprojected with the ray set-up's own unproject, pixel
centre and world-to-uvw map.  With fused=True the per-sample expressions are the fused ones of proj_ref.march / shadow_ref.march;
sigma, g(d) and with them S_near / S_far are separately rounded in both modes (ray placement).  Harness only."""
import numpy as np

import iso_ref as ir
import oracle_binding as ob
import proj_ref as pr
import shadow_ref as shr
import surf_ref as sr

f32 = np.float32
BASIC, LIGHT = 0, 1


def sigma(x, d):
    """(x.x*dir.x + x.y*dir.y) + x.z*dir.z, rows of (N, 3) float32 arrays."""
    with np.errstate(all="ignore"):
        return ((x[:, 0] * d[:, 0] + x[:, 1] * d[:, 1]) + x[:, 2] * d[:, 2]).astype(f32)


def g(u, W, H, px, py, d):
    """unproject(ndcx, ndcy, d) of the ray set-up for pixels (px, py) and depths d (arrays), mapped to texture space: (N, 3)."""
    px, py, d = np.asarray(px), np.asarray(py), np.asarray(d, f32)
    with np.errstate(all="ignore"):
        fx, fy = px.astype(f32) + f32(0.5), py.astype(f32) + f32(0.5)
        ndcx = (f32(2.0) * fx) / f32(W) - f32(1.0)
        ndcy = f32(1.0) - (f32(2.0) * fy) / f32(H)
        v = sr._mat_point(u.proj_inv, ndcx, ndcy, d, f32(1.0))
        w = sr._mat_point(u.view_inv, v[0] / v[3], v[1] / v[3], v[2] / v[3], f32(1.0))
        return np.stack([w[0] + f32(0.5), w[1] + f32(0.5), f32(0.5) - f32(2.0) * w[2]], -1).astype(f32)


def depth_of_world(u, xyz):
    """The depth convention: clip.z / clip.w of proj * view * (world, 1), the product of surf_ref.depth."""
    x, y, z = (f32(t) for t in xyz)
    e = sr._mat_point(u.view, x, y, z, f32(1.0))
    c = sr._mat_point(u.proj, e[0], e[1], e[2], e[3])
    return f32(c[2] / c[3])


def box_corner_depths(u):
    """(smallest, largest) depth of the eight corners of the volume's world box [-.5, .5]^2 x [-.25, .25]."""
    ds = [depth_of_world(u, (sx * 0.5, sy * 0.5, sz * 0.25)) for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]
    return min(ds), max(ds)


def march(variant, u, W, H, vec4, tf, near=None, far=None, pixels=None, fused=False):
    """BASIC or LIGHT between the bounds near / far (float32 [H, W] depth buffers, None = no bound on that side) for `pixels` (px, py)
    (default: the whole frame, row by row).  Returns a dict: frag (N, 4), composited (N,), covered (N,) = the ray goes through the
    box, pixels, and per pixel what the tests' pins need: before_far (N,) = steps of 0 .. steps_count-1 with sigma(p_k) < S_far,
    before_near (N,) = steps with !(sigma(p_k) >= S_near), prefix (N,) = those steps are the ray's first ones (sigma never steps back
    across a bound)."""
    assert variant in (BASIC, LIGHT)
    if pixels is None:
        pixels = np.stack(np.meshgrid(np.arange(W), np.arange(H)), -1).reshape(-1, 2)
    pixels = np.asarray(pixels, dtype=np.int64).reshape(-1, 2)
    vec4 = np.ascontiguousarray(np.asarray(vec4, dtype=f32))
    dens = np.ascontiguousarray(vec4[..., 3])
    opacity, color = (np.asarray(t, dtype=f32) for t in tf)
    N = len(pixels)
    out = dict(frag=np.zeros((N, 4), f32), composited=np.zeros(N, np.int64), covered=np.zeros(N, bool), pixels=pixels,
               before_far=np.zeros(N, np.int64), before_near=np.zeros(N, np.int64), prefix=np.ones(N, bool))
    start, end, world0 = (np.zeros((N, 3), f32) for _ in range(3))
    for k, (px, py) in enumerate(pixels):
        h, s, e, w = ob.setup_ray(u, W, H, int(px), int(py))
        out["covered"][k], start[k], end[k], world0[k] = h, s, e, w
    assert u.fragment_mode == 0
    idx = np.nonzero(out["covered"])[0]
    if idx.size == 0 or u.steps_count <= 0:
        return out
    M = idx.size
    with np.errstate(all="ignore"):
        diff = end[idx] - start[idx]
        ln = np.sqrt((diff[:, 0] * diff[:, 0] + diff[:, 1] * diff[:, 1]) + diff[:, 2] * diff[:, 2])
        dr = (diff * (f32(1.0) / ln)[:, None]).astype(f32)
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
    px, py = pixels[idx, 0], pixels[idx, 1]
    s_near = s_far = None
    if near is not None:
        s_near = sigma(g(u, W, H, px, py, np.asarray(near, f32).reshape(H, W)[py, px]), dr)
    if far is not None:
        s_far = sigma(g(u, W, H, px, py, np.asarray(far, f32).reshape(H, W)[py, px]), dr)
    w = world0[idx].copy()
    lo, hi = shr.clip_box(u)
    lpos, dif, amb = (np.asarray(a[:3], f32) for a in (u.light_pos, u.light_diffuse, u.light_ambient))
    n = np.zeros(M, np.int64)
    dst = np.zeros((M, 4), f32)
    b_far, b_near = np.zeros(M, np.int64), np.zeros(M, np.int64)
    prefix = np.ones(M, bool)
    past_near, past_far = np.zeros(M, bool), np.zeros(M, bool)
    for _ in range(u.steps_count):
        counts = np.all((p >= lo) & (p <= hi), axis=1)
        sg = sigma(p, dr)
        with np.errstate(all="ignore"):
            if s_near is not None:
                ok = sg >= s_near
                prefix &= ~(past_near & ~ok)
                past_near |= ok
                b_near += ~ok
                counts &= ok
            if s_far is not None:
                ok = sg < s_far
                prefix &= ~(past_far & ok)
                past_far |= ~ok
                b_far += ok
                counts &= ok
            mask = counts & ((dst[:, 3] <= f32(0.95)) if variant == BASIC else (dst[:, 3] < f32(1.0)))
        if mask.any():
            mi = np.nonzero(mask)[0]
            if variant == BASIC:
                o, rgb = pr.tf_lookup(opacity, color, pr.sample_a(dens, p[mi], fused), fused)
                col = rgb.astype(f32)
            else:
                v = ir.sample_rgba(vec4, p[mi], fused)
                o, rgb = pr.tf_lookup(opacity, color, np.ascontiguousarray(v[:, 3]), fused)
                sh = shr.shade_s(ir.normalize3(np.ascontiguousarray(v[:, :3]), fused), w[mi], lpos, dif, amb, 2.5, 0.5,
                                 np.ones(mi.size, f32), fused)
                with np.errstate(all="ignore"):
                    col = (rgb * sh).astype(f32)
            sub = dst[mi]
            pr._blend(col, o.astype(f32), sub, np.ones(mi.size, bool), fused)
            dst[mi] = sub
            n[mi] += 1
        with np.errstate(all="ignore"):
            p = p + step
            w = w + wstep
    out["frag"][idx] = dst
    out["composited"][idx] = n
    out["before_far"][idx], out["before_near"][idx], out["prefix"][idx] = b_far, b_near, prefix
    return out


def frame(variant, u, W, H, vec4, tf, near=None, far=None, fused=False):
    """(frag [H, W, 4], composited, covered) of the whole frame."""
    r = march(variant, u, W, H, vec4, tf, near, far, fused=fused)
    return r["frag"].reshape(H, W, 4), int(r["composited"].sum()), int(r["covered"].sum())
