"""float32 numpy restatement of vr_volume_resample (include/vr.h): the positions p = ((origin + i * di) + j * dj) + k * dk of the box's
voxels -- every operation rounded, or the three multiply-adds fused (fma_ref.fma32) --, the inside test (slice_ref.in_cube), the
linear sample (proj_ref.sample: texel pairs and seven lerps in the arithmetic mode) or the nearest voxel (slice_ref.nearest_index),
`outside` elsewhere, the components and voxels that keep their bits, the result and out[0]; and the float64 restatement of
vr_resample_between, operation by operation as the header orders them.  Harness only."""
import numpy as np

import proj_ref as pr
import slice_ref as sr
from fma_ref import mad

f32 = np.float32
LINEAR, NEAREST = 0, 1


def positions(origin, di, dj, dk, lo, hi, fused=False):
    """p (N, 3) of the voxels of the box lo <= (i, j, k) < hi, x fastest, and their (k, j, i) indices (N, 3)."""
    k, j, i = np.meshgrid(np.arange(lo[2], hi[2]), np.arange(lo[1], hi[1]), np.arange(lo[0], hi[0]), indexing="ij")
    k, j, i = k.ravel(), j.ravel(), i.ravel()
    o, di, dj, dk = (np.array(list(v), f32) for v in (origin, di, dj, dk))
    fi, fj, fk = i.astype(f32)[:, None], j.astype(f32)[:, None], k.astype(f32)[:, None]
    with np.errstate(all="ignore"):
        p = mad(fi, di[None, :], np.broadcast_to(o, (len(i), 3)).copy(), fused)
        p = mad(fj, dj[None, :], p, fused)
        p = mad(fk, dk[None, :], p, fused)
    return p.astype(f32), np.stack([k, j, i], -1)


def resample(src, dst, dst_n, channels, filt, origin, di, dj, dk, outside, lo, hi, fused=False):
    """(destination [nz, ny, nx, 4] float32, (inside, outside, lo, hi), box voxels, copied): `src` the source's voxels [nz, ny, nx, 4],
    `dst` the destination's before the call (None: an empty slot, created as zeros of dst_n = (nx, ny, nz)).  `copied` [nz, ny, nx, 4]
    is True where the stored bits are a copy -- untouched, `outside`, a NEAREST voxel -- and False where they come out of the lerps,
    whose NaNs carry no defined payload."""
    src = np.asarray(src, f32)
    nx, ny, nz = (int(v) for v in dst_n)
    out = np.zeros((nz, ny, nx, 4), f32) if dst is None else np.array(dst, f32, copy=True)
    assert out.shape == (nz, ny, nx, 4)
    copied = np.ones(out.shape, bool)
    box = int(np.prod([max(h - l, 0) for l, h in zip(lo, hi)]))
    if box == 0:
        return out, (0, 0, (0, 0, 0), (0, 0, 0)), 0, copied
    p, kji = positions(origin, di, dj, dk, lo, hi, fused)
    inside = sr.in_cube(p)
    val = np.broadcast_to(np.array(list(outside), f32), (len(p), 4)).copy()
    if inside.any():
        q = p[inside]
        if filt == NEAREST:
            k, j, i = sr.nearest_index(q, src.shape[:3])
            val[inside] = src[k, j, i]
        else:
            val[inside] = pr.sample(src, q, fused)
    sel = [c for c in range(4) if (channels >> c) & 1]
    k, j, i = kji[:, 0], kji[:, 1], kji[:, 2]
    ob, vb = out.view(np.uint32), val.view(np.uint32)
    for c in sel:
        ob[k, j, i, c] = vb[:, c]
        if filt == LINEAR:
            copied[k[inside], j[inside], i[inside], c] = False
    n_in = int(inside.sum())
    if n_in:
        w = kji[inside]
        blo = (int(w[:, 2].min()), int(w[:, 1].min()), int(w[:, 0].min()))
        bhi = (int(w[:, 2].max()) + 1, int(w[:, 1].max()) + 1, int(w[:, 0].max()) + 1)
    else:
        blo = bhi = (0, 0, 0)
    return out, (n_in, box - n_in, blo, bhi), box, copied


def resample_desc(src, dst, d, fused=False):
    """resample() of a capi.ResampleDesc."""
    return resample(src, dst, tuple(d.dst_n), int(d.channels), int(d.filter), tuple(d.origin), tuple(d.di), tuple(d.dj), tuple(d.dk),
                    tuple(d.outside), tuple(d.box_lo), tuple(d.box_hi), fused)


def identity(shape):
    """vr_resample_identity's geometry for a source of shape (nz, ny, nx): (dst_n, origin, di, dj, dk)."""
    nz, ny, nx = shape
    n = (nx, ny, nz)
    origin = tuple(f32(0.5) / f32(v) for v in n)
    z = f32(0.0)
    return n, origin, (f32(1.0) / f32(nx), z, z), (z, f32(1.0) / f32(ny), z), (z, z, f32(1.0) / f32(nz))


def between(src_n, src_origin, src_spacing, dst_n, dst_origin, dst_spacing, dst_to_src=None):
    """vr_resample_between in float64, the header's operations in the header's order: (origin, di, dj, dk), float32 (3,) each."""
    f64 = np.float64
    M = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], f64) if dst_to_src is None else np.asarray(dst_to_src, f64).reshape(3, 4)
    so, ss, do, ds = (np.asarray(v, f64) for v in (src_origin, src_spacing, dst_origin, dst_spacing))
    origin, di, dj, dk = (np.zeros(3, f32) for _ in range(4))
    with np.errstate(all="ignore"):
        for a in range(3):
            m = M[a]
            s = f64(1.0) / (ss[a] * f64(src_n[a]))
            v = ((((m[0] * do[0]) + (m[1] * do[1])) + (m[2] * do[2])) + m[3]) - so[a]
            origin[a] = f32((v * s) + (f64(0.5) / f64(src_n[a])))
            di[a] = f32((m[0] * ds[0]) * s)
            dj[a] = f32((m[1] * ds[1]) * s)
            dk[a] = f32((m[2] * ds[2]) * s)
    return origin, di, dj, dk


def same(got, want, copied):
    """The comparison of a downloaded destination with the restatement: every bit where the stored value is a copy; where it comes out
    of the lerps, NaN where the restatement has NaN and every bit elsewhere."""
    gb, wb = got.view(np.uint32), want.view(np.uint32)
    nan = np.isnan(want) & ~copied
    return bool(np.array_equal(gb[~nan], wb[~nan]) and np.isnan(got[nan]).all())
