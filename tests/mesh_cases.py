"""Inputs of the surface-extraction tests (vr_volume_mesh): the fields with known answers, volumes for the device tests, the sweep."""
import numpy as np

f32 = np.float32


def grid(n):
    """z, y, x index grids of an n = (nz, ny, nx) volume, relative to its centre."""
    nz, ny, nx = n
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return z - (nz - 1) / 2, y - (ny - 1) / 2, x - (nx - 1) / 2


def sphere(n=14, r=5.0):
    """r - |p - centre| on n^3: level 0 is a sphere of radius r."""
    z, y, x = grid((n, n, n))
    return (r - np.sqrt(x * x + y * y + z * z)).astype(f32)


def torus(n=14):
    """2 - hypot(hypot(x, y) - 4, z): level 0 is a torus of radii 4 and 2."""
    z, y, x = grid((n, n, n))
    return (2.0 - np.hypot(np.hypot(x, y) - 4.0, z)).astype(f32)


def one_voxel(n=5):
    v = np.zeros((n, n, n), f32)
    v[n // 2, n // 2, n // 2] = 1
    return v


def box_of_ones():
    return np.ones((3, 4, 5), f32)  # 5 x 4 x 3 (x, y, z)


def random_mask(shape=(6, 7, 9), p=0.5, seed=1):
    return (np.random.default_rng(seed).random(shape) < p).astype(f32)


def smooth_noise(shape, seed):
    """A few random plane waves: smooth, with level sets of every topology."""
    rng = np.random.default_rng(seed)
    nz, ny, nx = shape
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    v = np.zeros(shape)
    for _ in range(5):
        k = rng.normal(size=3) * 0.35
        v += rng.normal() * np.sin(k[0] * x + k[1] * y + k[2] * z + rng.uniform(0, 6.28))
    return v.astype(f32)


def vec4(channel_values, channel, seed=0):
    """A (nz, ny, nx, 4) float32 volume with the given component and arbitrary numbers in the others."""
    shape = channel_values.shape
    v = np.random.default_rng(seed).normal(size=shape + (4,)).astype(f32)
    v[..., channel] = channel_values
    return v


def random_box(rng, shape):
    """A box of the volume, sometimes flush with it, sometimes thin or empty: (lo, hi) in (x, y, z)."""
    lo, hi = [], []
    for n in shape[::-1]:
        kind = rng.integers(0, 8)
        if kind < 3:
            a, b = 0, n
        elif kind < 7:  # most of the axis
            a = int(rng.integers(0, n // 2 + 1))
            b = int(rng.integers(a + (n - a + 1) // 2, n + 1))
        else:  # thin or empty
            a = int(rng.integers(0, n))
            b = min(n, a + int(rng.integers(0, 3)))
        lo.append(a)
        hi.append(b)
    return tuple(lo), tuple(hi)


def sweep(count=40, seed=2024):
    """Seeded small random cases: thresholded smooth noise and random masks, random boxes, levels, caps, channels and kernel forms; at
    most 40 points per axis."""
    rng = np.random.default_rng(seed)
    cases = []
    for i in range(count):
        shape = tuple(int(rng.integers(1, 41)) for _ in range(3))
        if i % 5 == 0:
            shape = (int(rng.integers(1, 6)), int(rng.integers(1, 8)), int(rng.integers(30, 41)))
        if shape[0] * shape[1] * shape[2] > 12000:  # (the restatement is a Python loop over cells)
            shape = (max(1, 12000 // (shape[1] * shape[2])),) + shape[1:]
        kind = i % 3
        if kind == 0:
            v = smooth_noise(shape, seed + i)
            level = float(f32(rng.normal() * 0.5))
        elif kind == 1:
            v = (rng.random(shape) < rng.uniform(0.1, 0.9)).astype(f32)
            level = 0.5
        else:  # a few values only: many voxels equal to the level, constant bricks
            v = rng.integers(0, 3, size=shape).astype(f32)
            v[: shape[0] // 2] = f32(rng.integers(0, 3))
            level = float(rng.integers(0, 3))
        lo, hi = random_box(rng, shape)
        if i % 4 == 0:
            lo, hi = (0, 0, 0), shape[::-1]
        cases.append(dict(v=v, level=level, cap=int(rng.integers(0, 2)), channel=int(3 if i % 2 == 0 else rng.integers(0, 3)), box_lo=lo, box_hi=hi,
                          plain=bool(i % 7 == 3), seed=seed + i))
    return cases
