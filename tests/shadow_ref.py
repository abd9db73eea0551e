"""float32 numpy restatement of the shadows of include/vr.h (vr_set_shadows) in either arithmetic mode: the light volume's build
(texel centres, the walk toward the light by repeated rounded additions, BASIC's trilinear density and opacity look-up, the scale and
clamps, the early stop) and LIGHT's march with every blended sample's diffuse term scaled by the light volume's trilinear sample S.
Rays come from oracle_binding.setup_ray and the jitter from oracle_binding.jitter; the samplers, the look-ups and the blend are
proj_ref's and iso_ref's.  With fused=True the samplers' and look-ups' coordinates and lerps (of the volume, the tables and the light
volume), the dot products, the shading sum and the blend are single fused multiply-adds, as in the oracle's fused LIGHT; the light
volume's walk (l, c, D, len, dir, step, lim, q += step), s * a, T * (1 - a') and m * S are separately rounded in both modes.
Harness only."""
import numpy as np

import iso_ref as ir
import oracle_binding as ob
import proj_ref as pr

f32 = np.float32
LIGHT = 1
T_MIN = f32(2.0 ** -10)


def grid_of(shape_zyx, divisor):
    """(Gx, Gy, Gz) of a volume [nz, ny, nx(, 4)] at `divisor`."""
    nz, ny, nx = shape_zyx[:3]
    return tuple((n + divisor - 1) // divisor for n in (nx, ny, nz))


def clip_box(u):
    """IsInSampleCoords bounds (lo, hi) of uniforms u, as the shaders compute them."""
    lo = np.array([f32(0.0) + f32(u.clip_x[0]), f32(0.0) + f32(u.clip_y[0]), f32(0.0) + f32(u.clip_z[0])], f32)
    hi = np.array([f32(1.0) - f32(u.clip_x[1]), f32(1.0) - f32(u.clip_y[1]), f32(1.0) - f32(u.clip_z[1])], f32)
    return lo, hi


def opacity_lookup(opacity, d, fused=False):
    """BASIC's opacity look-up (textureSample(tfOpacity, linear, d), clamp-to-edge)."""
    return pr.opacity_lookup(opacity, d, fused)


def build(vec4, opacity, divisor, sigma, light_pos, lo, hi, texels=None, fused=False):
    """The light volume: T per texel.  vec4 [nz, ny, nx, 4] (or the density plane [nz, ny, nx]); light_pos = the uniforms' world
    light position (x, y, z); lo / hi = the clip box (clip_box).  texels: (N, 3) integer (i, j, k) to compute (default: every texel;
    then the result is float32[Gz, Gy, Gx], else float32[N])."""
    v = np.asarray(vec4, dtype=f32)
    dens = np.ascontiguousarray(v[..., 3] if v.ndim == 4 else v)
    opacity = np.asarray(opacity, dtype=f32)
    gx, gy, gz = grid_of(dens.shape, divisor)
    full = texels is None
    if full:
        k, j, i = np.meshgrid(np.arange(gz), np.arange(gy), np.arange(gx), indexing="ij")
        texels = np.stack([i.ravel(), j.ravel(), k.ravel()], 1)
    texels = np.asarray(texels, dtype=np.int64).reshape(-1, 3)
    sigma = f32(sigma)
    L = np.asarray(light_pos, dtype=f32)[:3]
    lo, hi = np.asarray(lo, f32), np.asarray(hi, f32)
    with np.errstate(all="ignore"):
        l = np.array([L[0] + f32(0.5), L[1] + f32(0.5), f32(0.5) - f32(2.0) * L[2]], f32)
        h = f32(1.0) / f32(max(gx, gy, gz))
        c = np.stack([(texels[:, 0].astype(f32) + f32(0.5)) / f32(gx), (texels[:, 1].astype(f32) + f32(0.5)) / f32(gy),
                      (texels[:, 2].astype(f32) + f32(0.5)) / f32(gz)], 1).astype(f32)
        D = (l[None, :] - c).astype(f32)
        dd = (D[:, 0] * D[:, 0] + D[:, 1] * D[:, 1]) + D[:, 2] * D[:, 2]
        ln = np.sqrt(dd)
        s = (D * (f32(1.0) / np.sqrt(dd))[:, None]) * h
        lim = ln / h
        K = np.where(lim < f32(65536.0), np.nan_to_num(lim, nan=65536.0), 65536.0).astype(np.int64)
    T = np.ones(len(texels), f32)
    q = c.copy()
    still = np.all(s == 0.0, axis=1)  # (a direction of length 0: the texel never moves)
    live = K >= 1
    n = 0
    while live.any():
        n += 1
        idx = np.nonzero(live)[0]
        with np.errstate(all="ignore"):
            qi = (q[idx] + s[idx]).astype(f32)
        q[idx] = qi
        inside = np.all((qi >= f32(0.0)) & (qi <= f32(1.0)), axis=1)
        inclip = inside & np.all((qi >= lo) & (qi <= hi), axis=1)
        a = np.zeros(idx.size, f32)
        if inclip.any():
            d = pr.sample_a(dens, qi[inclip], fused)
            with np.errstate(all="ignore"):
                ai = sigma * opacity_lookup(opacity, d, fused)
                ai = np.where(ai > f32(1.0), f32(1.0), ai)
                ai = np.where(ai > f32(0.0), ai, f32(0.0)).astype(f32)
            a[inclip] = ai
            t = T[idx[inclip]] * (f32(1.0) - ai)
            T[idx[inclip]] = t.astype(f32)
        done = ~inside | (n >= K[idx]) | (inclip & (T[idx] < T_MIN))
        # a texel that does not move and whose sample is transparent keeps T for the rest of its K steps
        done |= still[idx] & (a == f32(0.0))
        live[idx[done]] = False
    return T.reshape(gz, gy, gx) if full else T


def shade_s(N, w, lpos, dif, amb, kD, kA, S, fused=False):
    """iso_ref.shade with the diffuse term dif * (m * S), m * S rounded first."""
    return ir.shade(N, w, lpos, dif, amb, kD, kA, fused, S=S)


def march(u, W, H, vec4, tf, shadow, pixels=None, fused=False):
    """LIGHT with shadows of `pixels` (px, py) (default: the whole frame, row by row), the light volume `shadow` float32[Gz, Gy, Gx]
    (None: S = 1, which is LIGHT).  Returns (frag (N, 4), composited (N,), covered (N,), pixels)."""
    if pixels is None:
        pixels = np.stack(np.meshgrid(np.arange(W), np.arange(H)), -1).reshape(-1, 2)
    pixels = np.asarray(pixels, dtype=np.int64).reshape(-1, 2)
    vec4 = np.ascontiguousarray(np.asarray(vec4, dtype=f32))
    opacity, color = (np.asarray(t, dtype=f32) for t in tf)
    grid = None if shadow is None else np.ascontiguousarray(np.asarray(shadow, dtype=f32))
    N = len(pixels)
    frag = np.zeros((N, 4), f32)
    comp = np.zeros(N, np.int64)
    start, end, world0 = (np.zeros((N, 3), f32) for _ in range(3))
    rayhit = np.zeros(N, bool)
    for k, (px, py) in enumerate(pixels):
        h, s, e, w = ob.setup_ray(u, W, H, int(px), int(py))
        rayhit[k], start[k], end[k], world0[k] = h, s, e, w
    assert u.fragment_mode == 0
    cov = rayhit.copy()
    idx = np.nonzero(rayhit)[0]
    if idx.size == 0 or u.steps_count <= 0:
        return frag, comp, cov, pixels
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
    lo, hi = clip_box(u)
    lpos, dif, amb = (np.asarray(a[:3], f32) for a in (u.light_pos, u.light_diffuse, u.light_ambient))
    n = np.zeros(M, np.int64)
    dst = np.zeros((M, 4), f32)
    for _ in range(u.steps_count):
        inb = np.all((p >= lo) & (p <= hi), axis=1)
        mask = inb & (dst[:, 3] < f32(1.0))
        if mask.any():
            mi = np.nonzero(mask)[0]
            v = ir.sample_rgba(vec4, p[mi], fused)
            o, rgb = pr.tf_lookup(opacity, color, np.ascontiguousarray(v[:, 3]), fused)
            Nn = ir.normalize3(np.ascontiguousarray(v[:, :3]), fused)
            S = np.ones(mi.size, f32) if grid is None else pr.sample_a(grid, p[mi], fused)
            sh = shade_s(Nn, w[mi], lpos, dif, amb, 2.5, 0.5, S, fused)
            with np.errstate(all="ignore"):
                col = (rgb * sh).astype(f32)
            sub = dst[mi]
            pr._blend(col, o.astype(f32), sub, np.ones(mi.size, bool), fused)
            dst[mi] = sub
            n[mi] += 1
        with np.errstate(all="ignore"):
            p = p + step
            w = w + wstep
    frag[idx] = dst
    comp[idx] = n
    return frag, comp, cov, pixels


def frame(u, W, H, vec4, tf, shadow, fused=False):
    """(frag [H, W, 4], composited, covered) of the whole frame."""
    frag, comp, cov, _ = march(u, W, H, vec4, tf, shadow, fused=fused)
    return frag.reshape(H, W, 4), int(comp.sum()), int(cov.sum())
