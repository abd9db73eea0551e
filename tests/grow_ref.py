"""Restatement of vr_segment_grow (include/vr.h) that shares nothing with the kernels' bit-brick formulation: a voxel-by-voxel
breadth-first search with a deque over a numpy Q computed with the same f32 comparisons.  Volumes are float32[nz, ny, nx, 4]; boxes
and seeds are (x, y, z) as in the descriptor."""
from collections import deque
from itertools import product

import numpy as np

f32 = np.float32
FACES, ALL = 6, 26
REPLACE, ADD = 0, 1


def offsets(connectivity):
    """The (dx, dy, dz) of a voxel's neighbours."""
    assert connectivity in (FACES, ALL)
    out = [d for d in product((-1, 0, 1), repeat=3) if d != (0, 0, 0)]
    if connectivity == FACES:
        out = [d for d in out if sum(1 for c in d if c) == 1]
    assert len(out) == connectivity
    return out


def qualifies(values, lo, hi, box_lo, box_hi):
    """Q as bool[nz, ny, nx]: inside the half-open box and v >= lo && v <= hi in f32 (NaN never does)."""
    v = np.asarray(values, f32)
    with np.errstate(invalid="ignore"):
        q = (v >= f32(lo)) & (v <= f32(hi))
    inside = np.zeros(v.shape, bool)
    inside[box_lo[2]:box_hi[2], box_lo[1]:box_hi[1], box_lo[0]:box_hi[0]] = True
    return q & inside


def region(q, seeds, connectivity):
    """R as bool[nz, ny, nx]: the voxels of q connected to a seed that lies in q."""
    nz, ny, nx = q.shape
    r = np.zeros(q.shape, bool)
    todo = deque()
    for x, y, z in seeds:
        if 0 <= x < nx and 0 <= y < ny and 0 <= z < nz and q[z, y, x] and not r[z, y, x]:
            r[z, y, x] = True
            todo.append((x, y, z))
    offs = offsets(connectivity)
    while todo:
        x, y, z = todo.popleft()
        for dx, dy, dz in offs:
            a, b, c = x + dx, y + dy, z + dz
            if 0 <= a < nx and 0 <= b < ny and 0 <= c < nz and q[c, b, a] and not r[c, b, a]:
                r[c, b, a] = True
                todo.append((a, b, c))
    return r


def bounding_box(r):
    """(lo, hi) of r as (x, y, z) triples, half open; zeros when r is empty."""
    if not r.any():
        return (0, 0, 0), (0, 0, 0)
    z, y, x = np.nonzero(r)
    return (int(x.min()), int(y.min()), int(z.min())), (int(x.max()) + 1, int(y.max()) + 1, int(z.max()) + 1)


def grow(values, mask, contour, lo, hi, connectivity, mode, box_lo, box_hi, seeds):
    """(new mask float32[nz, ny, nx, 4], voxels, (lo, hi) of R, voxels of the box, R, Q).  `values` is the channel's float32[nz, ny,
    nx]; `mask` the mask slot's voxels before the call, or None for an empty slot."""
    values = np.asarray(values, f32)
    q = qualifies(values, lo, hi, box_lo, box_hi)
    r = region(q, seeds, connectivity)
    out = np.zeros(values.shape + (4,), f32) if mask is None else np.array(mask, f32, copy=True)
    bits = out.view(np.uint32)
    one = np.array([1.0], f32).view(np.uint32)[0]
    if mode == REPLACE:
        bits[..., contour] = 0
    else:
        assert mode == ADD
    bits[..., contour][r] = one
    box = int(np.prod([max(0, int(h) - int(l)) for l, h in zip(box_lo, box_hi)]))
    return out, int(r.sum()), bounding_box(r), box, r, q
