"""Inputs shared by the CPU and GPU tests of distance maps (vr_mask_distance): the shapes and boxes of the word and line edges, the
operand sets, the spacings, the 40 cases of the random sweep.  The sets with pinholes, the hostile values and the arbitrary bits are
morph_cases'."""
import numpy as np

from morph_cases import arbitrary_bits, dense, hostile, sparse, whole  # noqa: F401  (re-exported: the tests take them from here)

f32 = np.float32
UNIT = (1, 1, 1)
MM = (1000, 1000, 3000)        # micrometres: 1 x 1 x 3 mm
WIDE = (21, 37, 130)           # (nz, ny, nx): three words along x, the last one partial
# (nz, ny, nx) of the word and line edges: 70 x 9 x 6, 130 x 37 x 21, 64 x 4 x 4 voxels, one row per slice, one voxel per row
EDGE_SHAPES = [(6, 9, 70), WIDE, (4, 4, 64), (5, 1, 70), (9, 6, 1)]
# the unit-spacing shapes the GPU tests use: their largest D2 is below 2^24 (test_distance.py: injectivity)
UNIT_SHAPES = EDGE_SHAPES + [(21, 37, 70), (32, 32, 32)]


def boxes(shape):
    """The whole volume, boxes aligned neither to 4 nor to 64, boxes that begin and end at a word border, an empty box and a box of
    one voxel."""
    nz, ny, nx = shape
    out = [whole(shape), ((min(1, nx - 1), min(1, ny - 1), min(1, nz - 1)), (max(nx - 1, 1), max(ny - 1, 1), max(nz - 1, 1))),
           ((nx // 2, 0, 0), (nx // 2 + 1, 1, 1)), ((min(3, nx), 0, 0), (min(3, nx), ny, nz)), ((max(nx - 3, 0), 0, 0), (nx, ny, min(2, nz)))]
    if nx > 64:
        out += [((61, min(2, ny - 1), 1), (67, ny, nz - 1)), ((64, 0, 0), (nx, ny, nz)), ((63, 0, 0), (65, min(3, ny), nz))]
    return out


def shell(shape, seed=5):
    """A hollow ellipsoidal shell, two to three voxels thick: an inside that is background."""
    z, y, x = np.meshgrid(*[(np.arange(n) + 0.5) / n - 0.5 for n in shape], indexing="ij")
    r = np.sqrt((x / 0.40) ** 2 + (y / 0.36) ** 2 + (z / 0.42) ** 2)
    return (r <= 1.0) & (r >= 0.72)


def points(shape, xyz):
    """The set of the given (x, y, z) voxels."""
    a = np.zeros(shape, bool)
    for x, y, z in xyz:
        a[z, y, x] = True
    return a


def corners(shape):
    """(x, y, z) of the eight corners of a volume and of x = 63 / 64 in its middle row (where it is that wide)."""
    nz, ny, nx = shape
    out = [(x, y, z) for x in (0, nx - 1) for y in (0, ny - 1) for z in (0, nz - 1)]
    return out + [(x, ny // 2, nz // 2) for x in (63, 64) if x < nx]


def operands(shape):
    """name -> set: empty, full, dense noise, a hollow shell."""
    return {"empty": np.zeros(shape, bool), "full": np.ones(shape, bool), "noise": np.random.default_rng(6).random(shape) < 0.5,
            "dense": dense(shape, seed=7), "shell": shell(shape)}


def sweep(n=40, seed=13):
    """The random sweep's cases: dicts of shape (nz, ny, nx) up to 130 x 37 x 21 voxels, box_lo / box_hi, spacing, limit, scale, mode, src /
    dst slot, contour and channel, fresh (the destination slot is empty before the call), probe (None or a contour of slot 1), layout, the
    kind of set and the seed of the volumes."""
    rng = np.random.default_rng(seed)
    cases = []
    for i in range(n):
        nx = int(rng.choice([rng.integers(60, 71), rng.integers(125, 131), rng.integers(1, 131)], p=[0.4, 0.4, 0.2]))
        ny, nz = int(rng.integers(1, 38)), int(rng.integers(1, 22))
        dims = (nx, ny, nz)
        lo = [int(rng.integers(0, d + 1)) for d in dims]
        hi = [int(rng.integers(l, d + 1)) for l, d in zip(lo, dims)]
        if i % 4 != 3:  # (a box that is most of the volume, so that the cases are not all slivers)
            lo = [int(rng.integers(0, d // 4 + 1)) for d in dims]
            hi = [d - int(rng.integers(0, d // 4 + 1)) for d in dims]
        spacing = [UNIT, MM, (977, 977, 2500), tuple(int(s) for s in rng.integers(1, 5001, 3))][int(rng.integers(0, 4))]
        reach = max(s * max(h - l, 1) for s, l, h in zip(spacing, lo, hi))
        limit = 0 if rng.random() < 0.5 else int(rng.integers(1, reach + 1))
        mode = int(rng.integers(0, 3))
        src_slot, dst_slot, fresh = [(0, 0, False), (0, 1, False), (1, 0, False), (0, 2, True)][int(rng.integers(0, 4))]
        probe = None if mode == 1 or rng.random() < 0.4 else int(rng.integers(0, 4))
        cases.append(dict(shape=(nz, ny, nx), box_lo=tuple(lo), box_hi=tuple(hi), spacing=spacing, limit=limit,
                          scale=float(f32([1.0, 0.001, 0.5, 3.0][int(rng.integers(0, 4))])), mode=mode, src_slot=src_slot, dst_slot=dst_slot,
                          fresh=fresh, src_contour=int(rng.integers(0, 4)), dst_channel=int(rng.integers(0, 4)), probe=probe,
                          layout=(0, 1, 3)[i % 3], kind=("dense", "sparse", "shell")[int(rng.integers(0, 3))], seed=2000 + i))
    return cases


def sweep_set(case):
    shape, seed = case["shape"], case["seed"]
    return dense(shape, seed=seed) if case["kind"] == "dense" else sparse(shape, seed=seed, p=0.01) if case["kind"] == "sparse" else shell(shape)
