"""float32 numpy restatement of the BASIC shader's march (separately rounded arithmetic, as the CPU oracle restates
BasicVolumeApp.wgsl fs_main) and, on the same sample positions, the intensity projections of include/vr.h
(MIP / MINIP / AVERAGE).  Rays come from oracle_binding.setup_ray and the jitter from oracle_binding.jitter; every
other operation follows the oracle's order: normalize3s, the step, texel pairs, the seven lerps, the TF look-ups and
FrontToBackBlend.  With fused=True the expressions include/vr.h names under VR_ARITH_FUSED -- the texture and table coordinates,
every lerp, the blend -- are single fused multiply-adds (fma_ref.fma32), as the oracle's fused mode evaluates them; ray placement
(the direction, the step, p += step) and AVERAGE's s + d and s / n are separately rounded in both modes.  Harness only."""
import numpy as np

import oracle_binding as ob
from fma_ref import mad

f32 = np.float32
BASIC, MIP, MINIP, AVERAGE = 0, 8, 9, 10


def _i32_sat(x0):
    """f32 -> i32, saturating, NaN -> 0 (the oracle's f2i)."""
    x = np.asarray(x0, dtype=np.float64)
    x = np.where(np.isnan(x), 0.0, np.clip(x, -2147483648.0, 2147483647.0))
    return x.astype(np.int64)


def _texel_pair(x0, n):
    t = np.minimum(_i32_sat(x0), n - 1)
    return np.clip(t, 0, n - 1), np.clip(t + 1, 0, n - 1)


def _lerp(a, b, t, fused=False):
    with np.errstate(all="ignore"):
        return mad(b - a, t, a, fused)


def sample(vol, p, fused=False):
    """textureSample(vol, linear, p) for points p (N, 3) in either arithmetic mode: vol is a plane [nz, ny, nx] (the result is (N,))
    or the voxels [nz, ny, nx, C] (the result is (N, C)); clamp-to-edge texel pairs, the seven lerps x, then y, then z."""
    nz, ny, nx = vol.shape[:3]
    with np.errstate(all="ignore"):
        x = mad(p[:, 0], f32(nx), f32(-0.5), fused)
        y = mad(p[:, 1], f32(ny), f32(-0.5), fused)
        z = mad(p[:, 2], f32(nz), f32(-0.5), fused)
        x0, y0, z0 = np.floor(x), np.floor(y), np.floor(z)
        fx, fy, fz = x - x0, y - y0, z - z0
        if vol.ndim == 4:
            fx, fy, fz = fx[:, None], fy[:, None], fz[:, None]
        i0, i1 = _texel_pair(x0, nx)
        j0, j1 = _texel_pair(y0, ny)
        k0, k1 = _texel_pair(z0, nz)
        c00 = _lerp(vol[k0, j0, i0], vol[k0, j0, i1], fx, fused)
        c10 = _lerp(vol[k0, j1, i0], vol[k0, j1, i1], fx, fused)
        c01 = _lerp(vol[k1, j0, i0], vol[k1, j0, i1], fx, fused)
        c11 = _lerp(vol[k1, j1, i0], vol[k1, j1, i1], fx, fused)
        return _lerp(_lerp(c00, c10, fy, fused), _lerp(c01, c11, fy, fused), fz, fused)


def sample_a(dens, p, fused=False):
    """textureSample(vol, linear, p).a for points p (N, 3); dens is the .a plane [nz, ny, nx] (float32)."""
    return sample(dens, p, fused)


def opacity_lookup(opacity, d, fused=False):
    """textureSample(tfOpacity, linear, d) with clamp-to-edge: BASIC's opacity look-up of densities d."""
    with np.errstate(all="ignore"):
        x = mad(d, f32(opacity.size), f32(-0.5), fused)
        x0 = np.floor(x)
        i0, i1 = _texel_pair(x0, opacity.size)
        return _lerp(opacity[i0], opacity[i1], x - x0, fused)


def tf_lookup(opacity, color, d, fused=False):
    """(opacity, rgb) of densities d: textureSample(tfOpacity / tfColor, linear, d) with clamp-to-edge."""
    o = opacity_lookup(opacity, d, fused)
    with np.errstate(all="ignore"):
        xc = mad(d, f32(color.shape[0]), f32(-0.5), fused)
        xc0 = np.floor(xc)
        c0, c1 = _texel_pair(xc0, color.shape[0])
        rgb = _lerp(color[c0, :3], color[c1, :3], (xc - xc0)[:, None], fused)
    return o, rgb


def _blend(rgb, a, dst, mask, fused=False):
    """FrontToBackBlend: mad(1 - dst.a, src, dst) per channel, src = (rgb * a, a) (the products rgb * a rounded on their own)."""
    with np.errstate(all="ignore"):
        s = rgb * a[:, None]
        om = f32(1.0) - dst[:, 3]
        new = np.empty_like(dst)
        new[:, :3] = mad(om[:, None], s, dst[:, :3], fused)
        new[:, 3] = mad(om, a, dst[:, 3], fused)
    dst[mask] = new[mask]


def march(variant, u, W, H, vec4, tf, pixels=None, fused=False):
    """Returns (frag (N, 4), composited (N,), covered (N,), pixels (N, 2)) of BASIC or of a projection, for `pixels` (px, py)
    (default: the whole frame, row by row), in separately rounded or fused arithmetic."""
    if pixels is None:
        pixels = np.stack(np.meshgrid(np.arange(W), np.arange(H)), -1).reshape(-1, 2)
    pixels = np.asarray(pixels, dtype=np.int64).reshape(-1, 2)
    dens = np.ascontiguousarray(np.asarray(vec4, dtype=f32)[..., 3])
    opacity, color = (np.asarray(t, dtype=f32) for t in tf)
    N = len(pixels)
    frag = np.zeros((N, 4), f32)
    comp = np.zeros(N, np.int64)
    cov = np.zeros(N, bool)
    start = np.zeros((N, 3), f32)
    end = np.zeros((N, 3), f32)
    hit = np.zeros(N, bool)
    for k, (px, py) in enumerate(pixels):
        h, s, e, _ = ob.setup_ray(u, W, H, int(px), int(py))
        hit[k], start[k], end[k] = h, s, e
    assert u.fragment_mode == 0
    idx = np.nonzero(hit)[0]
    if variant == BASIC:
        cov[idx] = True
    if idx.size == 0 or u.steps_count <= 0:
        return frag, comp, cov, pixels
    with np.errstate(all="ignore"):
        diff = end[idx] - start[idx]
        ln = np.sqrt((diff[:, 0] * diff[:, 0] + diff[:, 1] * diff[:, 1]) + diff[:, 2] * diff[:, 2])
        inv = f32(1.0) / ln
        dr = diff * inv[:, None]
        ss = np.full(idx.size, f32(u.step_size), f32)
        if u.toggles[0] == 1:
            ss = ln / f32(u.steps_count)
        p = start[idx].copy()
        if u.toggles[1] == 1:
            j = np.array([ob.jitter(float(f32(px) + f32(0.5)), float(f32(py) + f32(0.5))) for px, py in pixels[idx]], f32)
            p = p + (dr * ss[:, None]) * j[:, None]
        step = dr * ss[:, None]
    lo = np.array([f32(0.0) + f32(u.clip_x[0]), f32(0.0) + f32(u.clip_y[0]), f32(0.0) + f32(u.clip_z[0])], f32)
    hi = np.array([f32(1.0) - f32(u.clip_x[1]), f32(1.0) - f32(u.clip_y[1]), f32(1.0) - f32(u.clip_z[1])], f32)
    n = np.zeros(idx.size, np.int64)
    dst = np.zeros((idx.size, 4), f32)
    m = np.full(idx.size, {MIP: -np.inf, MINIP: np.inf}.get(variant, 0.0), f32)
    for _ in range(u.steps_count):
        inb = np.all((p >= lo) & (p <= hi), axis=1)
        d = sample_a(dens, p, fused)
        if variant == BASIC:
            o, rgb = tf_lookup(opacity, color, d, fused)
            mask = inb & (dst[:, 3] <= f32(0.95))
            _blend(rgb, o, dst, mask, fused)
            n += mask
        else:
            n += inb
            if variant == MIP:
                m = np.where(inb & (d > m), d, m)
            elif variant == MINIP:
                m = np.where(inb & (d < m), d, m)
            else:
                with np.errstate(all="ignore"):
                    m = np.where(inb, m + d, m)
        with np.errstate(all="ignore"):
            p = p + step
    if variant != BASIC:
        v = m
        if variant == AVERAGE:
            with np.errstate(all="ignore"):
                v = m / np.maximum(n, 1).astype(f32)
        o, rgb = tf_lookup(opacity, color, v, fused)
        _blend(rgb, o, dst, n > 0, fused)
        cov[idx] = n > 0
    frag[idx] = dst
    comp[idx] = n
    return frag, comp, cov, pixels


def frame(variant, u, W, H, vec4, tf, fused=False):
    """(frag [H, W, 4], composited, covered) of the whole frame."""
    frag, comp, cov, _ = march(variant, u, W, H, vec4, tf, fused=fused)
    return frag.reshape(H, W, 4), int(comp.sum()), int(cov.sum())
