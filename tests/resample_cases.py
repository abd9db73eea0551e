"""Shapes, volumes, transforms, boxes and the random sweep of the resampling tests (tests/test_resample.py, tests/test_resample_gpu.py).
A transform is (origin, di, dj, dk) in the source's texture space, made by resample_ref.between from two patient-space grids, so the
cases are the geometry a caller has.  Harness only."""
import math

import numpy as np

import resample_ref as rr

f32 = np.float32
SRC_SHAPES = [(5, 9, 70), (6, 7, 1), (1, 1, 1)]      # (nz, ny, nx)
DST_SHAPES = [(7, 6, 130), (3, 5, 64), (2, 1, 65)]   # x: two wavefront units and a tail, exactly one unit, one voxel over
POW2 = (32, 16, 8)                                   # 8 x 16 x 32 voxels: the identity law holds
SRC_SPACING = (0.9, 1.1, 2.5)                        # x, y, z in millimetres
SRC_ORIGIN = (-31.0, 12.5, 3.0)
CHANNELS = [15, 8, 1, 5]
BOTH = ["magnify4", "minify3", "rot30z", "oblique"]  # transforms meant to leave voxels inside and voxels outside
ALL_INSIDE, ALL_OUTSIDE = ["zero"], ["nan", "far"]
HOSTILE_OUTSIDE = (float("nan"), -0.0, float("-inf"), 1e-42)


def n_of(shape):
    """(nx, ny, nz) of a (nz, ny, nx) shape."""
    return shape[2], shape[1], shape[0]


def volume(shape, seed):
    """Finite values of moderate size in every component."""
    return np.random.default_rng(seed).normal(0.0, 1.0, shape + (4,)).astype(f32)


def hostile(shape, seed):
    """A volume a fifth of whose components are NaN, +-inf, -0.0f, +0.0f, denormals or huge; the rest as volume()."""
    rng = np.random.default_rng(seed)
    v = volume(shape, seed + 1)
    special = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-42, -3e-45, 3e38, -3e38, 1.0], f32)
    pick = rng.random(v.shape) < 0.2
    v[pick] = special[rng.integers(0, len(special), int(pick.sum()))]
    return v


def arbitrary_bits(shape, seed):
    """A vec4 volume of arbitrary 32-bit words (NaN payloads included): what a destination may hold before the call."""
    return np.random.default_rng(seed).integers(0, 1 << 32, shape + (4,), dtype=np.uint64).astype(np.uint32).view(f32)


def rotation(axis, degrees):
    """The 3 x 3 rotation by `degrees` about `axis` (Rodrigues), float64."""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], np.float64)
    t = math.radians(degrees)
    return np.eye(3) + math.sin(t) * K + (1.0 - math.cos(t)) * (K @ K)


def grids(name, src_shape, dst_shape):
    """(src grid, dst grid, dst_to_src or None) of transform `name`: a grid = (n, origin, spacing) in patient millimetres."""
    sn, dn = n_of(src_shape), n_of(dst_shape)
    so, ss = np.array(SRC_ORIGIN), np.array(SRC_SPACING)
    centre = so + ss * (np.array(sn) - 1) / 2.0
    m = None
    if name == "magnify4":  # the dose case: a grid four times as fine, a sub-voxel offset, its first voxels before the source
        ds = ss / 4.0
        do = so + ss * np.array([-1.3, 0.2, -0.4])
    elif name == "minify3":
        ds = ss * 3.0
        do = so + ss * np.array([-2.5, 0.3, -0.6])
    elif name in ("rot30z", "oblique"):  # about the source's centre, a grid a fifth larger than the source's extent
        R = rotation((0, 0, 1), 30.0) if name == "rot30z" else rotation((1, 1, 1), 40.0)
        ds = ss * np.array(sn) / np.array(dn) * 1.2
        do = centre - ds * (np.array(dn) - 1) / 2.0
        m = np.concatenate([R, (centre - R @ centre)[:, None]], axis=1)
    else:
        raise KeyError(name)
    return (sn, tuple(so), tuple(ss)), (dn, tuple(do), tuple(ds)), m


def transform(name, src_shape, dst_shape):
    """(origin, di, dj, dk) as float32 (3,) arrays."""
    if name == "zero":  # every voxel at one point inside the source
        z = np.zeros(3, f32)
        return np.array([0.3, 0.45, 0.6], f32), z, z, z
    if name in ("nan", "far"):  # the identity's steps from an origin with a NaN, or at 1e30
        _, o, di, dj, dk = rr.identity(dst_shape)
        o = np.array(o, f32)
        o[1 if name == "nan" else 0] = f32(np.nan) if name == "nan" else f32(1e30)
        return o, np.array(di, f32), np.array(dj, f32), np.array(dk, f32)
    s, d, m = grids(name, src_shape, dst_shape)
    return rr.between(*s, *d, m)


def boxes(dst_shape):
    """Boxes (lo, hi) of a destination: the whole grid, one aligned to nothing, an empty one, one voxel."""
    nx, ny, nz = n_of(dst_shape)
    odd = ((min(3, nx - 1), min(1, ny - 1), min(1, nz - 1)), (max(nx - 2, min(3, nx - 1) + 1), ny, nz))
    return [((0, 0, 0), (nx, ny, nz)), odd, ((min(2, nx), 0, 0), (min(2, nx), ny, nz)), ((nx - 1, ny - 1, nz - 1), (nx, ny, nz))]


def settle_source():
    """(nz, ny, nx) = (16, 16, 80), .a in slabs along x: a non-zero constant, +0, mixed +-0, a slab with one NaN, noise; .rgb noise."""
    shape = (16, 16, 80)
    rng = np.random.default_rng(31)
    v = volume(shape, 32)
    a = v[..., 3]
    a[:, :, 0:16] = f32(2.5)
    a[:, :, 16:32] = f32(0.0)
    a[:, :, 32:48] = np.where(rng.random((16, 16, 16)) < 0.5, f32(0.0), f32(-0.0))
    a[:, :, 48:60] = f32(-0.0)
    a[7, 9, 53] = f32(np.nan)
    return v


def sweep(n=36, seed=17):
    """The random sweep: dicts of src / dst shape, transform (a named one, its twelve numbers perturbed), channels, filter, box, outside,
    arithmetic mode, flavour, layout, fresh destination and the volumes' seeds."""
    rng = np.random.default_rng(seed)
    names = BOTH + ALL_INSIDE + ALL_OUTSIDE
    cases = []
    for i in range(n):
        src_shape = SRC_SHAPES[int(rng.integers(0, 3))] if i % 3 else SRC_SHAPES[0]
        dst_shape = DST_SHAPES[int(rng.integers(0, 3))]
        name = names[i % len(names)]
        o, di, dj, dk = (np.array(v, f32) for v in transform(name, src_shape, dst_shape))
        if name in BOTH:
            o = (o + rng.normal(0, 0.02, 3)).astype(f32)
            di, dj, dk = ((v * (1.0 + rng.normal(0, 0.05, 3))).astype(f32) for v in (di, dj, dk))
        nx, ny, nz = n_of(dst_shape)
        lo = [int(rng.integers(0, m + 1)) for m in (nx, ny, nz)]
        hi = [int(rng.integers(l, m + 1)) for l, m in zip(lo, (nx, ny, nz))]
        if i % 4 == 0:
            lo, hi = [0, 0, 0], [nx, ny, nz]
        cases.append(dict(src_shape=src_shape, dst_shape=dst_shape, name=name, origin=o, di=di, dj=dj, dk=dk,
                          channels=int(rng.integers(1, 16)) if i % 5 else 8, filter=int(rng.integers(0, 2)), box_lo=tuple(lo), box_hi=tuple(hi),
                          outside=HOSTILE_OUTSIDE if i % 2 else tuple(float(x) for x in rng.normal(0, 1, 4)), fused=bool(i % 2),
                          flavour=int(rng.integers(0, 2)), layout=(0, 3, 1)[int(rng.integers(0, 3))], fresh=bool(rng.integers(0, 2)),
                          hostile=bool(rng.integers(0, 2)), seed=1000 + 3 * i))
    return cases
