"""Inputs shared by the CPU and GPU tests of connected components (vr_mask_components): seeded sets, masks with hostile values, the 40
cases of the random sweep and the hand-made shapes that break labellers."""
import numpy as np

import comp_ref as cr
import morph_cases as mc

f32 = np.float32
CONNECTIVITIES = [cr.FACES, cr.ALL, cr.PLANE_FACES, cr.PLANE_ALL]
NX = [1, 63, 64, 65, 130, 200]
DENSITIES = [0.05, 0.15, 0.3, 0.32, 0.35, 0.5, 0.7, 0.95]


def whole(shape):
    """The box of a whole (nz, ny, nx) volume."""
    return (0, 0, 0), (shape[2], shape[1], shape[0])


def random_set(shape, p, seed):
    return np.random.default_rng(seed).random(shape) < p


def volume(a, contour, seed):
    """A vec4 volume whose component `contour` has exactly the voxels of `a` in the contour (NaN, -inf, denormals inside, +0.0f and
    -0.0f outside) and arbitrary bits in the other three (morph_cases.hostile)."""
    return mc.hostile(a, contour, seed)


def sweep(n=40, seed=21):
    """The random sweep's cases: dicts of shape (nz, ny, nx), density, box, connectivity, background, the filters, the destinations
    (None: not asked for), combine, src / written slot, fresh (the written slot is empty before the call) and the volumes' seed.  The
    first 24 walk through nx x connectivity and the densities in turn, so that every one of them occurs whatever the seed."""
    rng = np.random.default_rng(seed)
    cases = []
    for i in range(n):
        nx = NX[i % 6]
        ny, nz = [(9, 5), (1, 7), (12, 1), (23, 11), (2, 2), (17, 6), (1, 1), (31, 3)][(i // 2) % 8]
        dims = (nx, ny, nz)
        density = DENSITIES[i % 8]
        connectivity = CONNECTIVITIES[(i // 6) % 4]
        background = int(i % 5 == 3)
        if i % 3 == 1:  # a box smaller than the volume (set voxels lie outside it: the density is everywhere)
            lo = [int(rng.integers(0, d // 3 + 1)) for d in dims]
            hi = [d - int(rng.integers(0, d // 3 + 1)) for d in dims]
        else:
            lo, hi = [0, 0, 0], list(dims)
        mode = i % 8  # what is written
        dst_contour = None if mode in (0, 5) else int(rng.integers(0, 4))
        label_channel = None if mode in (0, 2, 6) else int(rng.integers(0, 4))
        src_contour = int(rng.integers(0, 4))
        src_slot, dst_slot, fresh = [(0, 1, False), (0, 2, True), (0, 0, False), (1, 0, False)][i % 4]
        if mode == 0:
            dst_slot, fresh = None, False
        in_place = dst_slot == src_slot and i % 8 == 2  # dst == src, slot and contour
        if in_place:
            dst_contour = src_contour
        if dst_contour is not None and label_channel == dst_contour:
            label_channel = (label_channel + 1) % 4
        filt = dict(min_voxels=1, max_voxels=cr.U64_MAX, reject_faces=0, keep_largest=0)
        kind = i % 7
        if kind == 1:
            filt.update(min_voxels=int(rng.integers(2, 6)))
        elif kind == 2:
            filt.update(keep_largest=int(rng.integers(1, 4)))  # (small components abound: the K-th size is tied)
        elif kind == 3:
            filt.update(reject_faces=int(rng.integers(1, 64)))
        elif kind == 4:
            filt.update(min_voxels=7, max_voxels=3)  # a window that selects nothing
        elif kind == 5:
            filt.update(max_voxels=int(rng.integers(1, 4)), keep_largest=cr.MAX_KEEP)
        elif kind == 6:
            filt.update(min_voxels=1 << 40)  # nothing is that large
        cases.append(dict(shape=(nz, ny, nx), density=density, box_lo=tuple(lo), box_hi=tuple(hi), connectivity=connectivity,
                          background=background, src_slot=src_slot, src_contour=src_contour, dst_slot=dst_slot, fresh=fresh,
                          dst_contour=dst_contour, label_channel=label_channel, combine=int(i // 2 % 4), seed=3000 + i, **filt))
    return cases


def case_volumes(c):
    """(the source slot's voxels, the written slot's before the call or None)"""
    src = volume(random_set(c["shape"], c["density"], c["seed"]), c["src_contour"], c["seed"] + 1)
    if c["dst_slot"] is None or c["fresh"]:
        return src, None
    if c["dst_slot"] == c["src_slot"]:
        return src, src
    return src, mc.arbitrary_bits(c["shape"], c["seed"] + 2)


def reference(c, src, before):
    return cr.components(src, before, c["src_contour"], c["background"], c["connectivity"], c["box_lo"], c["box_hi"], c["min_voxels"],
                         c["max_voxels"], c["reject_faces"], c["keep_largest"], c["dst_contour"], c["combine"], c["label_channel"])


# ---- hand-made shapes --------------------------------------------------------------------------------------------------------------

def serpentine(shape=(5, 9, 130)):
    """One 6-connected path through the whole volume: every other row is full, joined to the next full row at alternating ends; every
    other slice likewise, joined through one voxel."""
    nz, ny, nx = shape
    a = np.zeros(shape, bool)
    for z in range(0, nz, 2):
        for y in range(0, ny, 2):
            a[z, y, :] = True
            if y + 2 < ny:
                a[z, y + 1, nx - 1 if (y // 2) % 2 == 0 else 0] = True
        if z + 2 < nz:
            a[z + 1, 0 if (z // 2) % 2 == 0 else ny - 1 - (ny - 1) % 2, 0] = True
    return a


def comb(shape=(3, 12, 70), axis="row"):
    """Teeth that meet only in the last row (axis "row": columns along y in one slice each) or only in the last slice ("slice")."""
    nz, ny, nx = shape
    a = np.zeros(shape, bool)
    if axis == "row":
        a[:, :, ::2] = True
        a[:, ny - 1, :] = True
        a[1::2] = False
    else:
        a[:, ::2, ::2] = True
        a[nz - 1] = True
    return a


def checkerboard(shape=(4, 5, 66)):
    z, y, x = np.indices(shape)
    return (x + y + z) % 2 == 0


def shells(n=13):
    """Nested cubic shells: the voxels at Chebyshev distance 5, 3 and 1 from the centre: holes within holes, the centre voxel the innermost."""
    z, y, x = np.indices((n, n, n))
    d = np.maximum(np.maximum(abs(x - n // 2), abs(y - n // 2)), abs(z - n // 2))
    return (d == 5) | (d == 3) | (d == 1)


def corner_pair(shape=(2, 3, 130)):
    """Two voxels that touch only at a corner across the word border at x = 63 / 64."""
    a = np.zeros(shape, bool)
    a[0, 1, 63] = True
    a[1, 2, 64] = True
    return a
