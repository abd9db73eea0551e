"""Restatement of the exact distance maps of a mask contour (vr_mask_distance, include/vr.h) in numpy: the semantics written down
directly, for the tests to compare the device against.  Volumes are (nz, ny, nx, 4) float32; boxes are ((x, y, z) lo, (x, y, z) hi), half
open; spacings are (sx, sy, sz) integers.  Squared distances are exact int64 (below 2^62 by the rules of the header); BEYOND marks a
voxel whose set of sources is empty or, with a limit, farther than the limit.  tests/test_distance.py pins d2_field to
scipy.ndimage.distance_transform_edt and to the two laws that tie it to morph_ref."""
import numpy as np

OUTSIDE, INSIDE, SIGNED = range(3)
BEYOND = np.int64(np.iinfo(np.int64).max)
U64_MAX = (1 << 64) - 1
MAX_SPACING, MAX_LIMIT, MAX_EXTENT = 1 << 20, 1 << 31, 1 << 30


def member(component):
    """Membership of a float32 component: != 0.0f, so NaN is in and -0.0f is out."""
    return component != np.float32(0.0)


def legal(box_lo, box_hi, spacing, limit=0):
    """The header's rules for spacing, limit and the extent of the box."""
    return (all(1 <= int(s) <= MAX_SPACING for s in spacing) and 0 <= int(limit) <= MAX_LIMIT and
            all((int(h) - int(l)) * int(s) <= MAX_EXTENT for l, h, s in zip(box_lo, box_hi, spacing)))


def d2_field(src, spacing):
    """min over the set voxels q of `src` (bool, (nz, ny, nx): the box's crop) of sum_a ((p_a - q_a) * s_a)^2, int64, BEYOND where src is
    empty.  Three separable min-plus passes: per axis, for every offset d, out = min(out, shifted(in, d) + (d * s)^2).  While the passes
    run "no source" is 2^62, above every distance the header's rules admit, so that adding an offset's (d * s)^2 <= 2^60 cannot wrap."""
    none = np.int64(1) << 62
    out = np.where(src, np.int64(0), none)
    for axis, s in ((2, int(spacing[0])), (1, int(spacing[1])), (0, int(spacing[2]))):
        n = out.shape[axis]
        cur = np.ascontiguousarray(np.moveaxis(out, axis, 0))
        new = cur.copy()
        tmp = np.empty_like(cur)
        for d in range(1, n):
            add = np.int64((d * s) ** 2)
            np.add(cur[:n - d], add, out=tmp[:n - d])
            np.minimum(new[d:], tmp[:n - d], out=new[d:])      # from the voxels d below
            np.add(cur[d:], add, out=tmp[:n - d])
            np.minimum(new[:n - d], tmp[:n - d], out=new[:n - d])  # ... and d above
        out = np.moveaxis(new, 0, axis)  # (a minimum that took part stays <= 2^62: `new` starts as `cur`)
    return np.ascontiguousarray(np.where(out >= none, BEYOND, out))


def d2_from_points(shape, points, spacing):
    """The same field of a few set voxels given as (x, y, z), by the definition itself: the minimum over the points.  For long axes,
    where the passes of d2_field would take offsets times voxels."""
    nz, ny, nx = shape
    z, y, x = np.meshgrid(np.arange(nz, dtype=np.int64), np.arange(ny, dtype=np.int64), np.arange(nx, dtype=np.int64), indexing="ij")
    out = np.full(shape, BEYOND, np.int64)
    sx, sy, sz = (int(s) for s in spacing)
    for px, py, pz in points:
        np.minimum(out, ((x - px) * sx) ** 2 + ((y - py) * sy) ** 2 + ((z - pz) * sz) ** 2, out=out)
    return out


def fields(a, spacing):
    """(D2out, D2in) of the box's crop `a` (bool): the distances to A' and to B' = box \\ A'."""
    return d2_field(a, spacing), d2_field(~a, spacing)


def limited(d2, limit):
    """With a limit L a value greater than L^2 becomes BEYOND (0: none)."""
    return d2 if not limit else np.where(d2 > np.int64(int(limit) ** 2), BEYOND, d2)


def magnitude(d2, limit, scale):
    """The stored magnitude: sqrt_rn((float)D2) * scale in float32; BEYOND gives (float)L * scale with a limit, +inf without one."""
    scale = np.float32(scale)
    finite = np.where(d2 == BEYOND, np.int64(0), d2)
    m = np.sqrt(finite.astype(np.float32)) * scale
    beyond = np.float32(int(limit)) * scale if limit else np.float32(np.inf)
    return np.where(d2 == BEYOND, beyond, m).astype(np.float32)


def stored(a, d2out, d2in, mode, limit, scale):
    """(the f32 values the mode stores over the crop, the voxels that store BEYOND's value)."""
    d2out, d2in = limited(d2out, limit), limited(d2in, limit)
    if mode == OUTSIDE:
        sel, sign = d2out, np.float32(1.0)
    elif mode == INSIDE:
        sel, sign = d2in, np.float32(1.0)
    elif mode == SIGNED:
        sel, sign = np.where(a, d2in, d2out), np.where(a, np.float32(-1.0), np.float32(1.0))
    else:
        raise ValueError(mode)
    return (magnitude(sel, limit, scale) * sign).astype(np.float32), int((sel == BEYOND).sum())


def distance(src, dst, src_contour, dst_channel, mode, box_lo, box_hi, spacing, limit=0, scale=1.0, probe=None, probe_contour=0, d2=None):
    """One vr_mask_distance.  src: the source slot's voxels; dst: the destination slot's before the call (None: an empty slot; pass src
    itself for dst_slot == src_slot); probe: the probe slot's voxels or None; d2: (D2out, D2in) of the crop if the caller has them.
    Returns (the destination slot's voxels after the call, the result as DistResult.as_tuple gives it, the voxels of the box)."""
    assert legal(box_lo, box_hi, spacing, limit) and np.isfinite(scale) and scale > 0 and not (probe is not None and mode == INSIDE)
    nz, ny, nx = src.shape[:3]
    (x0, y0, z0), (x1, y1, z1) = box_lo, box_hi
    crop = (slice(z0, z1), slice(y0, y1), slice(x0, x1))
    a = member(src[..., src_contour])[crop]
    d2out, d2in = d2 if d2 is not None else fields(a, spacing)
    out = np.zeros((nz, ny, nx, 4), np.float32) if dst is None else dst.copy()
    values, beyond = stored(a, d2out, d2in, mode, limit, scale)
    out[..., dst_channel][crop] = values  # (a view: the other three components and the outside of the box keep their bits)
    voxels = int(a.sum())
    if voxels:
        zz, yy, xx = np.nonzero(a)
        lo = (x0 + int(xx.min()), y0 + int(yy.min()), z0 + int(zz.min()))
        hi = (x0 + int(xx.max()) + 1, y0 + int(yy.max()) + 1, z0 + int(zz.max()) + 1)
    else:
        lo = hi = (0, 0, 0)
    n_probe = p_min = p_max = 0
    if probe is not None:
        p = member(probe[..., probe_contour])[crop]
        n_probe = int(p.sum())
        if n_probe:
            at = limited(d2out, limit)[p]
            at = [U64_MAX if v == BEYOND else int(v) for v in (at.min(), at.max())]
            p_min, p_max = at
    return out, (voxels, lo, hi, beyond, n_probe, p_min, p_max), int(a.size)
