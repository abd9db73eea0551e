"""Inputs shared by the CPU and GPU tests of contour tracing (vr_mask_outlines): small slices with known outlines, masks as float32
voxels whose members are given, a sequential crack walker that states the definition of include/vr.h edge by edge, and the 40 cases of
the random sweep."""
import numpy as np

import raster_cases as rc

GRIDS = rc.GRIDS


def offsets(spacing):
    """The three offsets the tests use on a grid: 0, spacing - 1 and spacing / 2 rounded down."""
    return [(0, 0), (spacing[0] - 1, spacing[1] - 1), (spacing[0] // 2, spacing[1] // 2)]


def slices_with_known_outlines():
    """(name, boolean (ny, nx) slice, polygons under SPLIT, polygons under JOIN, points under SPLIT, points under JOIN)."""
    def z(ny, nx, *cells):
        s = np.zeros((ny, nx), bool)
        for x, y in cells:
            s[y, x] = True
        return s

    full = np.ones((5, 7), bool)
    hole = np.ones((5, 5), bool)
    hole[2, 2] = False
    board = (np.add.outer(np.arange(6), np.arange(6)) & 1) == 0
    return [("single_voxel", z(3, 3, (1, 1)), 1, 1, 4, 4),
            ("full_slice", full, 1, 1, 4, 4),
            ("one_voxel_hole", hole, 2, 2, 8, 8),
            ("diagonal", z(4, 4, (1, 1), (2, 2)), 2, 1, 8, 8),
            ("anti_diagonal", z(4, 4, (2, 1), (1, 2)), 2, 1, 8, 8),
            ("checkerboard", board, 18, None, 72, 72)]


def volume(m, seed=0):
    """Float32 voxels (nz, ny, nx, 4) whose members are the boolean (4, nz, ny, nx) m: members are 1.0, NaN, a denormal, -2.5 or +inf,
    the others +0.0 or -0.0."""
    rng = np.random.default_rng(seed)
    ins = np.array([1.0, np.nan, 1e-42, -2.5, np.inf], np.float32)
    outs = np.array([0.0, -0.0], np.float32)
    shape = m.shape[1:]
    v = np.zeros(shape + (4,), np.float32)
    for k in range(4):
        v[..., k] = np.where(m[k], ins[rng.integers(0, len(ins), shape)], outs[rng.integers(0, 2, shape)])
    return v


def random_members(shape, p, seed):
    """Boolean (4, nz, ny, nx), each voxel in with probability p."""
    return np.random.default_rng(seed).random((4,) + tuple(shape)) < p


def blobs(shape, seed, n=6):
    """Boolean (4, nz, ny, nx): a few overlapping discs and rectangles per contour and slice, some with holes."""
    rng = np.random.default_rng(seed)
    nz, ny, nx = shape
    yy, xx = np.mgrid[0:ny, 0:nx]
    m = np.zeros((4,) + tuple(shape), bool)
    for k in range(4):
        for z in range(nz):
            for _ in range(n):
                cx, cy, r = rng.uniform(0, nx), rng.uniform(0, ny), rng.uniform(1, 0.4 * max(nx, ny))
                disc = (xx - cx) ** 2 + (yy - cy) ** 2 <= r * r
                if rng.random() < 0.4:
                    m[k, z] &= ~disc
                else:
                    m[k, z] |= disc
    return m


def walk(s, connect, nx_lattice=None):
    """The definition, edge by edge, on one boolean (ny, nx) slice: every crack as (key -> head vertex), successors by the turn rule,
    loops followed from the smallest unvisited key.  Returns a list of polygons, each a list of lattice vertices (i, j), in the order
    of the definition."""
    ny, nx = s.shape
    n1 = (nx if nx_lattice is None else nx_lattice) + 1
    step = [(1, 0), (0, 1), (-1, 0), (0, -1)]

    def inside(x, y):
        return 0 <= x < nx and 0 <= y < ny and bool(s[y, x])

    tails = {}  # key -> (i, j, direction)
    for y, x in np.argwhere(s):
        x, y = int(x), int(y)
        for d, (tx, ty), (ox, oy) in ((0, (x, y), (x, y - 1)), (1, (x + 1, y), (x + 1, y)), (2, (x + 1, y + 1), (x, y + 1)), (3, (x, y + 1), (x - 1, y))):
            if not inside(ox, oy):
                tails[(ty * n1 + tx) * 4 + d] = (tx, ty, d)

    def successor(key):
        i, j, d = tails[key]
        hi, hj = i + step[d][0], j + step[d][1]
        leaving = [e for e in range(4) if (hj * n1 + hi) * 4 + e in tails]
        assert len(leaving) in (1, 2)
        e = leaving[0] if len(leaving) == 1 else (d + (3 if connect else 1)) & 3
        assert e in leaving
        return (hj * n1 + hi) * 4 + e

    seen, out = set(), []
    for key in sorted(tails):
        if key in seen:
            continue
        loop, k = [], key
        while k not in seen:
            seen.add(k)
            loop.append(k)
            k = successor(k)
        assert k == key
        pts = [tails[k][:2] for n, k in enumerate(loop) if tails[loop[n - 1]][2] != tails[k][2]]
        assert tails[loop[-1]][2] != tails[loop[0]][2]  # the first edge's tail is a corner
        out.append(pts)
    return out


def walk_volume(m, contours, connect, box_lo, box_hi, origin=(0, 0), spacing=(1, 1), offset=(0, 0)):
    """walk over every traced contour and slice of the box: (points int32 (N, 2), polygons [(first, count, slice, contour)])."""
    _, nz, ny, nx = m.shape
    inbox = np.zeros((ny, nx), bool)
    inbox[box_lo[1]:box_hi[1], box_lo[0]:box_hi[0]] = True
    polys = []
    for k in range(4):
        if not (contours >> k) & 1:
            continue
        for z in range(box_lo[2], box_hi[2]):
            for loop in walk(m[k, z] & inbox, connect):
                p = np.asarray(loop, np.int64)
                p = np.stack([origin[0] - offset[0] + p[:, 0] * spacing[0], origin[1] - offset[1] + p[:, 1] * spacing[1]], -1)
                polys.append((p, z, k))
    return rc.flatten(polys)


WORD_EDGE_SHAPES = [(6, 9, 70), (21, 37, 130), (4, 4, 64), (3, 5, 65)]


def edge_boxes(shape):
    """The boxes of test_raster_gpu.test_word_and_box_edges for a volume of `shape` (nz, ny, nx), cut to the volume (65 x 5 x 3 is
    smaller than the volumes of that test)."""
    nz, ny, nx = shape
    boxes = [((0, 0, 0), (nx, ny, nz)), ((1, 1, 1), (nx - 1, ny - 1, nz - 1)), ((nx // 2, 1, 0), (nx // 2 + 1, 2, 1)), ((3, 2, 1), (3, ny, nz)),
             ((nx - 3, 0, 0), (nx, ny, 2)), ((0, 0, nz - 1), (min(nx, 64), ny - 1, nz))]
    if nx > 64:
        boxes += [((61, 2, 1), (min(67, nx), ny - 2, nz - 1)), ((64, 0, 0), (nx, ny, nz)), ((63, 1, 0), (65, 3, nz))]
    return boxes


def sweep(n=40, seed=29):
    """The random sweep's cases: dicts of shape (nz, ny, nx), box_lo / box_hi, spacing, origin, offset, contours, connect, plain (the
    kernel form) and the members m."""
    rng = np.random.default_rng(seed)
    cases = []
    for i in range(n):
        nx = int(rng.choice([rng.integers(60, 71), rng.integers(125, 136), rng.integers(1, 141)], p=[0.4, 0.4, 0.2]))
        ny, nz = int(rng.integers(1, 90)), int(rng.integers(1, 9))
        dims = (nx, ny, nz)
        lo = [int(rng.integers(0, d + 1)) for d in dims]
        hi = [int(rng.integers(l, d + 1)) for l, d in zip(lo, dims)]
        if i % 4 != 1:  # (a box that is most of the volume, so that most cases are not slivers)
            lo = [int(rng.integers(0, d // 4 + 1)) for d in dims]
            hi = [d - int(rng.integers(0, d // 4 + 1)) for d in dims]
        spacing = [(1, 1), (977, 977), (500, 700), (1 << 20, 3), (int(rng.integers(1, 5000)), int(rng.integers(1, 5000)))][int(rng.integers(0, 5))]
        origin = (int(rng.integers(-300000, 300000)), int(rng.integers(-300000, 300000)))
        offset = tuple(int(rng.integers(0, s)) for s in spacing)
        kind = i % 3
        m = blobs((nz, ny, nx), 3000 + i) if kind == 0 else random_members((nz, ny, nx), [0.5, 0.15][kind - 1], 3000 + i)
        cases.append(dict(shape=(nz, ny, nx), box_lo=tuple(lo), box_hi=tuple(hi), spacing=spacing, origin=origin, offset=offset,
                          contours=int(rng.integers(1, 16)), connect=int(rng.integers(0, 2)), plain=bool(i % 2), m=m, seed=3000 + i))
    return cases
