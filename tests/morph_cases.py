"""Inputs shared by the CPU and GPU tests of mask morphology (vr_mask_morph): the issue's five balls, seeded sets, masks with hostile
values, the 40 cases of the random sweep, and the conversion between morph_ref's elements and the binding's."""
import numpy as np

import morph_ref as mr
from volumerendering_amd import capi

f32 = np.float32

# (spacing, radius) in micrometres; the last one has radii (31, 22, 17)
BALLS = [((1000, 1000, 3000), 5000), ((977, 977, 2500), 7000), ((1, 1, 1), 1), ((1, 1, 1), 5), ((500, 700, 900), 15500)]
REACH = ((500, 700, 900), 15500)


def whole(shape):
    """The box of a whole (nz, ny, nx) volume."""
    return (0, 0, 0), (shape[2], shape[1], shape[0])


def sparse(shape, seed=1, p=0.004):
    """A few isolated voxels."""
    return np.random.default_rng(seed).random(shape) < p


def dense(shape, seed=2):
    """A solid ellipsoid with pinholes (CLOSE has something to fill) among isolated specks (OPEN has something to remove)."""
    rng = np.random.default_rng(seed)
    z, y, x = np.meshgrid(*[(np.arange(n) + 0.5) / n - 0.5 for n in shape], indexing="ij")
    body = (x / 0.42) ** 2 + (y / 0.38) ** 2 + (z / 0.45) ** 2 <= 1.0
    return (body & (rng.random(shape) >= 0.04)) | (~body & (rng.random(shape) < 0.01))


def arbitrary_bits(shape, seed=3):
    """A vec4 volume of arbitrary bit patterns: a third of the components random 32-bit words (NaN payloads, denormals, negatives), the
    rest from a list of special values that holds -0.0f."""
    rng = np.random.default_rng(seed)
    special = np.array([0x00000000, 0x80000000, 0x3F800000, 0x7FC00001, 0xFFC12345, 0x7F800000, 0x00000001, 0xC0200000], np.uint32)
    bits = special[rng.integers(0, len(special), shape + (4,))]
    rnd = rng.integers(0, 1 << 32, shape + (4,), dtype=np.uint64).astype(np.uint32)
    return np.where(rng.random(shape + (4,)) < 0.33, rnd, bits).view(f32)


def hostile(a, contour, seed=4):
    """A vec4 volume whose component `contour` has exactly the voxels of `a` in the contour: NaN, 2.5f, 1.0f, -inf and a denormal inside,
    +0.0f and -0.0f outside; the other three components hold arbitrary bits."""
    rng = np.random.default_rng(seed)
    v = arbitrary_bits(a.shape, seed + 100).copy()
    inside = np.array([0x7FC00000, 0x40200000, 0x3F800000, 0xFF800000, 0x00000001, 0xFFC00321], np.uint32)
    outside = np.array([0x00000000, 0x80000000], np.uint32)
    comp = np.where(a, inside[rng.integers(0, len(inside), a.shape)], outside[rng.integers(0, len(outside), a.shape)])
    v[..., contour] = comp.view(f32)
    assert np.array_equal(mr.member(v[..., contour]), a)
    return v


def to_capi(element) -> capi.MorphElement:
    """morph_ref's (radii, half) as the binding's struct; entries outside the window are -1."""
    (rx, ry, rz), half = element
    e = capi.MorphElement()
    table = np.ctypeslib.as_array(e.half)
    table[:] = -1
    table[:2 * rz + 1, :2 * ry + 1] = half
    e.radius[:] = [rx, ry, rz]
    return e


def from_capi(e: capi.MorphElement):
    return tuple(int(r) for r in e.radius), e.table()


def ball_inputs(n=200, seed=7):
    """(spacing, radius) pairs with every quotient radius / spacing <= 31 and spacings up to 2^20."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        top = (1 << 20) if i % 3 == 0 else int(rng.choice([3, 40, 1000, 5000]))
        sp = tuple(int(s) for s in rng.integers(1, top + 1, 3))
        if i % 10 == 0:
            sp = (1 << 20,) + sp[1:]
        radius = int(rng.integers(0, 32 * min(sp)))  # (below 32 * the smallest spacing: every quotient is at most 31)
        out.append((sp, radius))
    return out


def sweep(n=40, seed=11):
    """The random sweep's cases: dicts of shape (nz, ny, nx), box_lo / box_hi, element, op, combine, src / dst slot and contour, fresh
    (the destination slot is empty before the call) and the seeds of the two volumes."""
    rng = np.random.default_rng(seed)
    cases = []
    for i in range(n):
        nx = int(rng.choice([rng.integers(60, 71), rng.integers(125, 136), rng.integers(1, 141)], p=[0.4, 0.4, 0.2]))
        ny, nz = int(rng.integers(1, 141)), int(rng.integers(1, 141))
        dims = (nx, ny, nz)
        lo = [int(rng.integers(0, d + 1)) for d in dims]
        hi = [int(rng.integers(l, d + 1)) for l, d in zip(lo, dims)]
        if i % 4 == 0:  # (a box that is most of the volume, so that big cases are not all slivers)
            lo = [int(rng.integers(0, d // 4 + 1)) for d in dims]
            hi = [d - int(rng.integers(0, d // 4 + 1)) for d in dims]
        cap = [min(mr.MAX_RADIUS, d) for d in dims]
        if rng.random() < 0.5:
            element = mr.box(*[int(rng.integers(0, c + 1)) for c in cap])
        else:
            sp = tuple(int(s) for s in rng.integers(300, 3001, 3))
            radius = int(rng.integers(0, min((c + 1) * s for c, s in zip(cap, sp))))  # (radius // s <= c on every axis)
            element = mr.ball(sp, radius)
        src_slot, dst_slot, fresh = [(0, 0, False), (0, 1, False), (1, 0, False), (0, 2, True)][int(rng.integers(0, 4))]
        cases.append(dict(shape=(nz, ny, nx), box_lo=tuple(lo), box_hi=tuple(hi), element=element, op=int(rng.integers(0, 5)),
                          combine=int(rng.integers(0, 4)), src_slot=src_slot, dst_slot=dst_slot, fresh=fresh,
                          src_contour=int(rng.integers(0, 4)), dst_contour=int(rng.integers(0, 4)), seed=1000 + i,
                          dense=bool(rng.random() < 0.5)))
    return cases
