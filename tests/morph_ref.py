"""Restatement of mask morphology and contour algebra (vr_mask_morph, include/vr.h) in numpy: the semantics written down directly, for
the tests to compare the device against.  Volumes are (nz, ny, nx, 4) float32; boxes are ((x, y, z) lo, (x, y, z) hi), half open; an
element is (radii (rx, ry, rz), half) with half an integer array [2 rz + 1][2 ry + 1] of half-chords along x, -1 for "no offset".
tests/test_morph.py pins dilate and erode to scipy.ndimage."""
import numpy as np

NONE, DILATE, ERODE, CLOSE, OPEN = range(5)
REPLACE, OR, AND, ANDNOT = range(4)
MAX_RADIUS = 31
ONE = np.uint32(0x3F800000)  # 1.0f


def ball(spacing, radius):
    """vr_morph_ball in int64: (dx, dy, dz) is in E iff (dx sx)^2 + (dy sy)^2 + (dz sz)^2 <= radius^2; radii = radius // spacing."""
    sx, sy, sz = (int(s) for s in spacing)
    rx, ry, rz = int(radius) // sx, int(radius) // sy, int(radius) // sz
    dz, dy, dx = np.meshgrid(np.arange(-rz, rz + 1, dtype=np.int64), np.arange(-ry, ry + 1, dtype=np.int64),
                             np.arange(0, rx + 1, dtype=np.int64), indexing="ij")
    inside = (dx * sx) ** 2 + (dy * sy) ** 2 + (dz * sz) ** 2 <= np.int64(radius) ** 2
    half = inside.sum(axis=2).astype(np.int64) - 1  # (inside is a prefix along dx: the terms grow with dx)
    return (rx, ry, rz), half.astype(np.int8)


def box(rx, ry, rz):
    """vr_morph_box: every half-chord of the window is rx."""
    return (rx, ry, rz), np.full((2 * rz + 1, 2 * ry + 1), rx, np.int8)


def valid(element):
    """The rules of include/vr.h for an element."""
    (rx, ry, rz), half = element
    if not all(0 <= r <= MAX_RADIUS for r in (rx, ry, rz)) or half.shape != (2 * rz + 1, 2 * ry + 1):
        return False
    return bool(half[rz, ry] >= 0 and (half >= -1).all() and (half <= rx).all() and np.array_equal(half, half[::-1]) and np.array_equal(half, half[:, ::-1]))


def structure(element):
    """The element as a boolean array [2 rz + 1][2 ry + 1][2 rx + 1] (what scipy.ndimage calls a structure)."""
    (rx, ry, rz), half = element
    dx = np.abs(np.arange(-rx, rx + 1))
    return dx[None, None, :] <= half[:, :, None].astype(np.int64)


def or_shifted(out, a, dx, dy, dz):
    """out[p] |= a[p - (dx, dy, dz)] wherever p - d lies inside the array (two slices: nothing wraps)."""
    nz, ny, nx = a.shape
    if abs(dx) >= nx or abs(dy) >= ny or abs(dz) >= nz:
        return
    dst = tuple(slice(max(d, 0), n + min(d, 0)) for d, n in ((dz, nz), (dy, ny), (dx, nx)))
    src = tuple(slice(max(-d, 0), n + min(-d, 0)) for d, n in ((dz, nz), (dy, ny), (dx, nx)))
    out[dst] |= a[src]


def dilate(a, element):
    """{ p in the array : p - e in a for some e in E }: the OR over the element's offsets, by slicing.  a: bool (nz, ny, nx), the box's
    crop.  The runs along x are formed once per half-chord (the run of half-chord h is that of h - 1 and the two offsets +-h)."""
    (rx, ry, rz), half = element
    runs = {0: a.copy()}
    for h in range(1, int(half.max()) + 1):
        runs[h] = runs[h - 1].copy()
        or_shifted(runs[h], a, h, 0, 0)
        or_shifted(runs[h], a, -h, 0, 0)
    out = np.zeros_like(a)
    for dz in range(-rz, rz + 1):
        for dy in range(-ry, ry + 1):
            h = int(half[dz + rz, dy + ry])
            if h >= 0:
                or_shifted(out, runs[h], 0, dy, dz)
    return out


def erode(a, element):
    """box \\ dilate(box \\ a): p survives iff every p + e that lies in the array is in a."""
    return ~dilate(~a, element)


def apply(op, a, element):
    if op == NONE:
        return a.copy()
    if op == DILATE:
        return dilate(a, element)
    if op == ERODE:
        return erode(a, element)
    if op == CLOSE:
        return erode(dilate(a, element), element)
    if op == OPEN:
        return dilate(erode(a, element), element)
    raise ValueError(op)


def member(component):
    """Membership of a float32 component: != 0.0f, so NaN is in and -0.0f is out."""
    return component != np.float32(0.0)


def morph(src, dst, src_contour, dst_contour, op, combine, box_lo, box_hi, element):
    """One vr_mask_morph.  src: the source slot's voxels; dst: the destination slot's before the call (None: an empty slot; pass src
    itself for dst_slot == src_slot).  Returns (the destination slot's voxels after the call, |R|, |A'|, (lo, hi) of R as (x, y, z)
    tuples, the voxels of the box, R as a boolean volume)."""
    nz, ny, nx = src.shape[:3]
    (x0, y0, z0), (x1, y1, z1) = box_lo, box_hi
    crop = (slice(z0, z1), slice(y0, y1), slice(x0, x1))
    a = member(src[..., src_contour])[crop]
    r = apply(op, a, element) if a.size else a.copy()
    out = np.zeros((nz, ny, nx, 4), np.float32) if dst is None else dst.copy()
    comp = out[..., dst_contour].view(np.uint32)  # (a view: writes go to `out`)
    cur = comp[crop]
    if combine == REPLACE:
        new = np.where(r, ONE, np.uint32(0))
    elif combine == OR:
        new = np.where(r, ONE, cur)
    elif combine == AND:
        new = np.where(r, cur, np.uint32(0))
    elif combine == ANDNOT:
        new = np.where(r, np.uint32(0), cur)
    else:
        raise ValueError(combine)
    comp[crop] = new
    full = np.zeros((nz, ny, nx), bool)
    full[crop] = r
    voxels = int(r.sum())
    if voxels:
        zz, yy, xx = np.nonzero(full)
        lo, hi = (int(xx.min()), int(yy.min()), int(zz.min())), (int(xx.max()) + 1, int(yy.max()) + 1, int(zz.max()) + 1)
    else:
        lo = hi = (0, 0, 0)
    return out, voxels, int(a.sum()), (lo, hi), int(a.size), full
