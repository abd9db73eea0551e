"""Inputs shared by the CPU and GPU tests of polygon rasterisation (vr_mask_polygons): polygons given in voxel coordinates (exact
rationals) and placed on a grid of any origin and spacing, the tie-rule shapes, a regular n-gon, a comb, a cloud of small polygons, and
the 40 cases of the random sweep."""
from fractions import Fraction as F

import numpy as np

# (spacing, origin): the unit grid, a CT pitch in micrometres off a negative origin, an anisotropic grid
GRIDS = [((1, 1), (0, 0)), ((977, 977), (-250000, -181333)), ((500, 700), (-1234, 77)), ((1, 1), (-40, -9))]


def place(voxel_points, origin, spacing):
    """Points given in voxel coordinates (numbers or Fractions; (0, 0) is the centre of voxel (0, 0)) as integer points of the grid's
    unit, rounded half up.  With an integer voxel coordinate the point is a voxel centre exactly."""
    out = []
    for vx, vy in voxel_points:
        out.append((origin[0] + int((F(vx) * spacing[0] + F(1, 2)).__floor__()), origin[1] + int((F(vy) * spacing[1] + F(1, 2)).__floor__())))
    return np.asarray(out, np.int64).reshape(-1, 2)


def flatten(polys):
    """[(points (n, 2), slice, contour), ...] -> (all points as int32 (N, 2), [(first, count, slice, contour), ...])."""
    pts, recs, first = [], [], 0
    for p, z, k in polys:
        p = np.asarray(p, np.int64).reshape(-1, 2)
        pts.append(p)
        recs.append((first, len(p), int(z), int(k)))
        first += len(p)
    allp = np.concatenate(pts) if pts else np.zeros((0, 2), np.int64)
    return allp.astype(np.int32), recs


def rect(x0, y0, x1, y1):
    return [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]


def ngon(n, cx, cy, rx, ry, phase=0.1):
    """A regular n-gon in voxel coordinates, its vertices rounded to 1/64 voxel."""
    t = phase + 2.0 * np.pi * np.arange(n) / n
    return [(F(int(round((cx + rx * np.cos(a)) * 64)), 64), F(int(round((cy + ry * np.sin(a)) * 64)), 64)) for a in t]


def comb(x0, y0, teeth, height):
    """A comb of `teeth` teeth, each one voxel wide with one voxel between them, 4 points per tooth: the teeth cover the centres
    x0 + 2 t, the back the row y0.  In voxel coordinates, edges half way between centres."""
    h = F(1, 2)
    pts = [(x0 - h, y0 - h)]
    for t in range(teeth):
        xa, xb = x0 + 2 * t - h, x0 + 2 * t + h
        pts += [(xa, y0 + h), (xa, y0 + height + h), (xb, y0 + height + h), (xb, y0 + h)]
    pts += [(x0 + 2 * teeth - 1 - h, y0 - h)]  # (below the last tooth's right side; the back closes to the first point)
    return pts


def tie_shapes():
    """The tie-rule shapes in voxel coordinates, as (name, points): vertices exactly on voxel centres, edges through centres, horizontal
    edges on centre rows, a polygon entirely between two centre rows, polygons of 1 and 2 points, zero area, a bow-tie."""
    return [
        ("rect_on_centres", rect(2, 1, 9, 6)),                                     # left / lower centres in, right / upper out
        ("triangle_on_centres", [(1, 1), (11, 1), (1, 11)]),                       # the hypotenuse passes through centres
        ("diamond_on_centres", [(6, 0), (12, 5), (6, 10), (0, 5)]),                # every vertex and many edge points on centres
        ("steep_through_centres", [(3, 0), (5, 8), (9, 8), (7, 0)]),               # edges of slope 4 through centres, horizontal on rows
        ("between_rows", [(1, F(9, 4)), (10, F(9, 4)), (10, F(11, 4)), (1, F(11, 4))]),  # no centre row inside
        ("between_columns", [(F(9, 4), 1), (F(11, 4), 1), (F(11, 4), 9), (F(9, 4), 9)]),
        ("one_point", [(4, 4)]),
        ("two_points", [(2, 2), (9, 7)]),
        ("zero_area", [(2, 2), (9, 7), (2, 2), (9, 7)]),
        ("bow_tie", [(1, 1), (11, 9), (11, 1), (1, 9)]),                           # self-intersecting: two triangles, even-odd
        ("bow_tie_overlap", [(1, 1), (11, 1), (3, 9), (3, 3), (9, 3), (9, 9)]),
        ("concave_with_flat_steps", [(0, 0), (4, 0), (4, 3), (8, 3), (8, 0), (12, 0), (12, 8), (6, 8), (6, 5), (0, 5)]),
        ("half_pixel_rect", rect(F(3, 2), F(3, 2), F(17, 2), F(13, 2))),
    ]


def cloud(n, shape_xy, seed, size=6):
    """n small overlapping polygons (3 .. 6 points) spread over nx x ny voxels, in voxel coordinates (quarters)."""
    rng = np.random.default_rng(seed)
    nx, ny = shape_xy
    out = []
    for _ in range(n):
        cx, cy = rng.uniform(0, nx), rng.uniform(0, ny)
        m = int(rng.integers(3, 7))
        out.append([(F(int(round((cx + rng.uniform(-size, size)) * 4)), 4), F(int(round((cy + rng.uniform(-size, size)) * 4)), 4)) for _ in range(m)])
    return out


def random_polygon(rng, nx, ny, n):
    """n points around a centre that may lie outside the grid, angles sorted half of the time (a star-shaped outline) and unsorted
    otherwise (self-intersecting), in voxel coordinates (eighths)."""
    cx, cy = rng.uniform(-0.2 * nx, 1.2 * nx), rng.uniform(-0.2 * ny, 1.2 * ny)
    r = rng.uniform(0.5, 0.6 * max(nx, ny))
    t = rng.uniform(0, 2 * np.pi, n)
    if rng.random() < 0.5:
        t = np.sort(t)
    rad = r * rng.uniform(0.3, 1.0, n)
    if rng.random() < 0.3:  # (snap to centres: ties)
        return [(int(round(cx + a * np.cos(b))), int(round(cy + a * np.sin(b)))) for a, b in zip(rad, t)]
    return [(F(int(round((cx + a * np.cos(b)) * 8)), 8), F(int(round((cy + a * np.sin(b)) * 8)), 8)) for a, b in zip(rad, t)]


def sweep(n=40, seed=19):
    """The random sweep's cases: dicts of shape (nz, ny, nx), spacing, origin, box_lo / box_hi, rule, combine, contours, grid_slot,
    dst_slot, fresh (the destination slot is empty before the call), points, polygons and the seed of the destination's bits."""
    rng = np.random.default_rng(seed)
    cases = []
    for i in range(n):
        nx = int(rng.choice([rng.integers(60, 71), rng.integers(125, 136), rng.integers(1, 141)], p=[0.4, 0.4, 0.2]))
        ny, nz = int(rng.integers(1, 141)), int(rng.integers(1, 25))
        dims = (nx, ny, nz)
        lo = [int(rng.integers(0, d + 1)) for d in dims]
        hi = [int(rng.integers(l, d + 1)) for l, d in zip(lo, dims)]
        if i % 4 != 1:  # (a box that is most of the volume, so that most cases are not slivers)
            lo = [int(rng.integers(0, d // 4 + 1)) for d in dims]
            hi = [d - int(rng.integers(0, d // 4 + 1)) for d in dims]
        spacing = [(1, 1), (977, 977), (500, 700), (1 << 20, 3), (int(rng.integers(1, 5000)), int(rng.integers(1, 5000)))][int(rng.integers(0, 5))]
        origin = (int(rng.integers(-300000, 300000)), int(rng.integers(-300000, 300000)))
        contours = int(rng.integers(1, 16))
        allowed = [k for k in range(4) if (contours >> k) & 1]
        n_poly = int(rng.integers(0, 61)) if i % 5 else 0
        polys = []
        for _ in range(n_poly):
            pts = place(random_polygon(rng, nx, ny, int(rng.integers(1, 91))), origin, spacing)
            polys.append((pts, int(rng.integers(-1, nz + 1)), int(rng.choice(allowed))))
        points, polygons = flatten(polys)
        grid_slot, dst_slot, fresh = [(0, 0, False), (0, 1, False), (1, 0, False), (0, 2, True)][int(rng.integers(0, 4))]
        cases.append(dict(shape=(nz, ny, nx), spacing=spacing, origin=origin, box_lo=tuple(lo), box_hi=tuple(hi), rule=int(rng.integers(0, 2)),
                          combine=int(rng.integers(0, 4)), contours=contours, grid_slot=grid_slot, dst_slot=dst_slot, fresh=fresh,
                          points=points, polygons=polygons, seed=2000 + i))
    return cases
