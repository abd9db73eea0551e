"""Volumes, bounds and seeds shared by the region-growing tests (test_grow.py on the CPU, test_grow_gpu.py on the device)."""
import numpy as np

import grow_ref as gr
import test_histogram_gpu as thg

f32 = np.float32
INF = float("inf")
SMALL = thg.SMALL            # (nz, ny, nx) = (13, 18, 23): no side a multiple of 4
LARGE = (40, 52, 72)         # several workgroups, a long frontier
QUANTILE = {gr.FACES: 0.35, gr.ALL: 0.12}  # just above the site-percolation thresholds of the two lattices (0.312, 0.098)


def whole(shape):
    nz, ny, nx = shape[:3]
    return (0, 0, 0), (nx, ny, nz)


def noise_case(shape, connectivity, seed=11):
    """(volume float32[nz, ny, nx, 4], lo, hi): thg.noise with its hostile values, hi at the connectivity's quantile of the numbers in
    .a, lo = -inf: one tortuous component among many small ones."""
    v = thg.noise(shape, seed=seed)
    a = v[..., 3]
    hi = f32(np.quantile(a[np.isfinite(a)].astype(np.float64), QUANTILE[connectivity]))
    return v, -INF, float(hi)


def seeds_from(q, n, seed, want=True):
    """n voxels (x, y, z) drawn from q (want = True) or from its complement."""
    z, y, x = np.nonzero(q if want else ~q)
    rng = np.random.default_rng(seed)
    pick = rng.choice(len(x), size=min(n, len(x)), replace=False)
    return [(int(x[i]), int(y[i]), int(z[i])) for i in pick]


def largest_component_seed(q, connectivity):
    """A voxel of the largest component of q (by the restatement: grows from every unreached voxel of q in turn)."""
    left = q.copy()
    best, best_n = None, 0
    while left.any():
        z, y, x = (int(t[0]) for t in np.nonzero(left))
        r = gr.region(left, [(x, y, z)], connectivity)
        if int(r.sum()) > best_n:
            best, best_n = (x, y, z), int(r.sum())
        left &= ~r
    return best, best_n


def snake(n=24):
    """A one-voxel-wide boustrophedon through the even rows of the even slices of an n^3 volume, linked at alternating ends: it
    visits every 4^3 brick in series.  Returns (.a float32[n, n, n], first voxel, last voxel, length)."""
    a = np.zeros((n, n, n), f32)
    path = []
    fwd_y = fwd_x = True
    for z in range(0, n, 2):
        rows = list(range(0, n, 2))
        if not fwd_y:
            rows.reverse()
        for k, y in enumerate(rows):
            xs = list(range(n)) if fwd_x else list(range(n - 1, -1, -1))
            path += [(x, y, z) for x in xs]
            if k + 1 < len(rows):  # the link to the next row, at this row's end
                path.append((xs[-1], y + (1 if fwd_y else -1), z))
            fwd_x = not fwd_x
        if z + 2 < n:  # the link to the next even slice, at this slice's end
            path.append((path[-1][0], path[-1][1], z + 1))
        fwd_y = not fwd_y
    for x, y, z in path:
        a[z, y, x] = 1.0
    assert len(set(path)) == len(path)
    assert all(sum(abs(p - q) for p, q in zip(a0, a1)) == 1 for a0, a1 in zip(path, path[1:]))
    return a, path[0], path[-1], len(path)
