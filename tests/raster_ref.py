"""The restatement of polygon rasterisation (vr_mask_polygons, include/vr.h) in int64 numpy, formulated as the kernels work: per row
and edge, an edge that counts on a row toggles the voxels [0, k) of the row, k = clamp(ceil(N / D), 0, nx), and a polygon's row is the
parity of the toggles at or above each voxel.  With the combine and the result boxes.  tests/test_raster.py pins it against an independent
per-voxel crossing count in exact rationals."""
import numpy as np

EVEN_ODD, UNION = 0, 1
REPLACE, OR, AND, ANDNOT = range(4)
ONE = np.uint32(0x3F800000)
MAX_COORD, MAX_SPACING = 1 << 29, 1 << 20


def edge_k(ax, ay, bx, by, yc, ox, sx, nx):
    """The k of one edge on the row of centre ordinate yc, or None if the edge does not count there.  Python integers."""
    if ay > by:
        ax, ay, bx, by = bx, by, ax, ay
    if not (ay <= yc < by):
        return None
    n = (yc - ay) * (bx - ax) + (ax - ox) * (by - ay)
    d = sx * (by - ay)
    return min(max(-((-n) // d), 0), nx)


def polygon_rows(points, origin, spacing, nx, ny):
    """The voxels one polygon covers on a slice of nx x ny voxels: a boolean (ny, nx) array.  points: (n, 2) integers."""
    p = np.asarray(points, np.int64).reshape(-1, 2)
    out = np.zeros((ny, nx), bool)
    if len(p) == 0 or nx == 0 or ny == 0:
        return out
    q = np.roll(p, -1, axis=0)
    up = p[:, 1] <= q[:, 1]
    ax, ay = np.where(up, p[:, 0], q[:, 0]), np.where(up, p[:, 1], q[:, 1])
    bx, by = np.where(up, q[:, 0], p[:, 0]), np.where(up, q[:, 1], p[:, 1])
    (ox, oy), (sx, sy) = (int(v) for v in origin), (int(v) for v in spacing)
    yc = (oy + np.arange(ny, dtype=np.int64) * sy)[:, None]                      # (ny, 1)
    counts = (ay[None, :] <= yc) & (yc < by[None, :])                            # (ny, edges); by > ay where it holds
    n = (yc - ay[None, :]) * (bx - ax)[None, :] + ((ax - ox) * (by - ay))[None, :]
    d = np.where(counts, sx * (by - ay)[None, :], 1)
    k = np.clip(-((-n) // d), 0, nx)                                             # ceil(n / d), clamped
    toggles = np.zeros((ny, nx + 1), np.int64)                                   # toggles[j, k]: edges of row j with that k
    rows = np.broadcast_to(np.arange(ny)[:, None], k.shape)
    np.add.at(toggles, (rows[counts], k[counts]), 1)
    upto = np.cumsum(toggles, axis=1)                                            # edges with k <= x
    above = upto[:, -1:] - upto[:, :nx]                                          # edges with k > x: those that toggle voxel x
    return (above & 1).astype(bool)


def sets(shape, points, polygons, origin, spacing, rule, box_lo, box_hi):
    """R_0 .. R_3 as boolean (4, nz, ny, nx): the polygons (first, count, slice, contour) of each contour on their slices, combined by
    `rule`, cut to the box."""
    nz, ny, nx = shape
    pts = np.asarray(points, np.int64).reshape(-1, 2)
    r = np.zeros((4, nz, ny, nx), bool)
    for first, count, z, contour in polygons:
        if not (box_lo[2] <= z < box_hi[2]):
            continue
        rows = polygon_rows(pts[first:first + count], origin, spacing, nx, ny)
        if rule == EVEN_ODD:
            r[contour, z] ^= rows
        else:
            r[contour, z] |= rows
    inbox = np.zeros((nz, ny, nx), bool)
    inbox[box_lo[2]:box_hi[2], box_lo[1]:box_hi[1], box_lo[0]:box_hi[0]] = True
    return r & inbox[None]


def count_box(r):
    """(|r|, lo, hi) of a boolean (nz, ny, nx) set: the half-open bounding box as (x, y, z) tuples, zeros when empty."""
    voxels = int(r.sum())
    if not voxels:
        return 0, (0, 0, 0), (0, 0, 0)
    zz, yy, xx = np.nonzero(r)
    return voxels, (int(xx.min()), int(yy.min()), int(zz.min())), (int(xx.max()) + 1, int(yy.max()) + 1, int(zz.max()) + 1)


def raster(shape, dst, points, polygons, origin, spacing, contours, rule, combine, box_lo, box_hi):
    """One vr_mask_polygons on a grid of `shape` (nz, ny, nx).  dst: the destination slot's voxels before the call (None: an empty
    slot).  Returns (the destination slot's voxels after the call, the result as PolygonsResult.as_tuple gives it, R as (4, nz, ny, nx))."""
    nz, ny, nx = shape
    for _, _, _, contour in polygons:
        assert (contours >> contour) & 1
    r = sets(shape, points, polygons, origin, spacing, rule, box_lo, box_hi)
    out = np.zeros((nz, ny, nx, 4), np.float32) if dst is None else dst.copy()
    crop = (slice(box_lo[2], box_hi[2]), slice(box_lo[1], box_hi[1]), slice(box_lo[0], box_hi[0]))
    result = []
    for k in range(4):
        if not (contours >> k) & 1:
            assert not r[k].any()
            result.append((0, (0, 0, 0), (0, 0, 0)))
            continue
        comp = out[..., k].view(np.uint32)  # (a view: writes go to `out`)
        cur, rk = comp[crop], r[k][crop]
        if combine == REPLACE:
            new = np.where(rk, ONE, np.uint32(0))
        elif combine == OR:
            new = np.where(rk, ONE, cur)
        elif combine == AND:
            new = np.where(rk, cur, np.uint32(0))
        elif combine == ANDNOT:
            new = np.where(rk, np.uint32(0), cur)
        else:
            raise ValueError(combine)
        comp[crop] = new
        result.append(count_box(r[k]))
    return out, tuple(result), r
