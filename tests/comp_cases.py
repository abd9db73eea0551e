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


# ---- scale: the sizes at which the kernels take another path (tests/test_components.py checks each against its header) --------------

SCAN_TILE = 1024                    # kScanTile (csrc/vr_scan.h): elements per workgroup of a scan
SPINE_CHUNK = 256                   # tiles per round of scan_spine_kernel's loop (csrc/vr_scan.h): one chunk = 262 144 elements
TOOL_BLOCKS = 512                   # kToolBlocks (csrc/vr_api_tools.h)
LANE_CAP = 4 * TOOL_BLOCKS * 256    # lane_blocks (csrc/vr_api_tools.h): lanes of a comp_* launch; beyond it the loops go round
WORDS_PER_PASS = TOOL_BLOCKS * 4    # tool_blocks (csrc/vr_api_tools.h): words of the box per round of the pack and of the write
AXIS = 65535                        # the longest axis of a volume

RODS = {"x": (1, 3, AXIS), "y": (2, AXIS, 3), "z": (AXIS, 3, 2), "xx": (3, 3, AXIS)}


def rod_axis(name):
    """The long axis of a rod as an index into (x, y, z)."""
    return "xyz".index(name[0])


def rod(name, seed=11):
    """A volume with one axis of 65535 (RODS).  x rods, by row in turn: the full row [0, 65534]; a row with the run [0, 63], seeded
    specks and the voxel 65534; every other voxel from 0 (32 768 runs, one of them [64, 64], the last [65534, 65534]); an empty row; a
    seeded row of density 0.3 behind a run that starts at 64; every other voxel from 1; a seeded row of density 0.5; an empty row; the
    second row again with another seed.  The full row touches the second row (and, in "xx", an empty one): what the specks join is one
    component through it, the isolated voxels of the third row stay apart.  y and z rods: three columns that touch at corners only -- a
    full one, every other voxel, a seeded one of density 0.5."""
    shape = RODS[name]
    rng = np.random.default_rng(seed)
    a = np.zeros(shape, bool)
    if name[0] == "x":
        rows = a.reshape(-1, AXIS)
        for r in range(rows.shape[0]):
            kind = r % 9
            if kind == 0:
                rows[r] = True
            elif kind in (1, 8):
                rows[r, :64] = True
                rows[r, 70:65500] = rng.random(65430) < 0.01
                rows[r, AXIS - 1] = True
            elif kind == 2:
                rows[r, ::2] = True
            elif kind == 4:
                rows[r, 64:200] = True
                rows[r, 201:] = rng.random(AXIS - 201) < 0.3
            elif kind == 5:
                rows[r, 1::2] = True
            elif kind == 6:
                rows[r] = rng.random(AXIS) < 0.5
        return a
    columns = np.moveaxis(a, 0 if name == "z" else 1, -1)  # (a view: [short, short, long])
    columns[0, 0] = True
    if name == "y":  # (z, x): (0, 0), (0, 2), (1, 1)
        columns[0, 2, ::2] = True
        columns[1, 1] = rng.random(AXIS) < 0.5
    else:            # (y, x): (0, 0), (2, 0), (1, 1)
        columns[2, 0, ::2] = True
        columns[1, 1] = rng.random(AXIS) < 0.5
    return a


def rod_boxes(name):
    """The whole box, and the box that cuts one voxel off each end of the long axis."""
    lo, hi = whole(RODS[name])
    cut_lo, cut_hi = list(lo), list(hi)
    cut_lo[rod_axis(name)] += 1
    cut_hi[rod_axis(name)] -= 1
    return [(lo, hi), (tuple(cut_lo), tuple(cut_hi))]


def columns(shape=(128, 128, 128)):
    a = np.zeros(shape, bool)
    a[:, :, ::2] = True
    return a


# name -> (set, connectivity, keep_largest): 128^3 is 32 MiB a slot, the blobs' (90, 128, 256) 45 MiB -- 64 slices of them have 393 112
# nodes, below LANE_CAP; 90 have 553 693 and cost the restatement 3 s
MIDDLE = {"checkerboard_faces": (lambda: checkerboard((128, 128, 128)), cr.FACES, 64),
          "checkerboard_all": (lambda: checkerboard((128, 128, 128)), cr.ALL, 1),
          "columns": (lambda: columns(), cr.FACES, 3),
          "blobs": (lambda: random_set((90, 128, 256), 0.25, 4242), cr.FACES, 5)}

SCAN_SHAPE = (512, 545, 8)  # one word a row
SCAN_BOXES = {"one_chunk": ((0, 0, 0), (8, 512, 512)), "one_more": ((0, 0, 0), (8, 545, 481))}
SCAN_DENSITY, SCAN_SEED = 0.3, 515


def box_words(shape, box_lo, box_hi):
    """The words of a box: the 64-voxel words of a row that meet [box_lo[0], box_hi[0]), times its rows and slices."""
    if any(h <= l for l, h in zip(box_lo, box_hi)):
        return 0
    return ((box_hi[0] - 1) // 64 - box_lo[0] // 64 + 1) * (box_hi[1] - box_lo[1]) * (box_hi[2] - box_lo[2])


def reference_arrays(src, dst, src_contour, background, connectivity, box_lo, box_hi, min_voxels=1, max_voxels=cr.U64_MAX, reject_faces=0,
                     keep_largest=0, dst_contour=None, combine=cr.REPLACE, label_channel=None):
    """comp_ref.components without a loop over components, for masks with a million of them: the same dict, but `table` is
    comp_ref.table_arrays' five arrays and `selected` an array.  tests/test_components.py pins it to comp_ref.components on the sweep."""
    nz, ny, nx = src.shape[:3]
    (x0, y0, z0), (x1, y1, z1) = box_lo, box_hi
    crop = (slice(z0, z1), slice(y0, y1), slice(x0, x1))
    s = cr.member(src[..., src_contour])[crop]
    if background:
        s = ~s
    lab, n = cr.label(s, connectivity)
    tab = cr.table_arrays(lab, n, box_lo)
    voxels, faces = tab[0], tab[4]
    sel = np.flatnonzero((voxels >= min_voxels) & (voxels <= min(max_voxels, (1 << 63) - 1)) & ((faces & reject_faces) == 0))
    if keep_largest:
        sel = np.sort(sel[np.lexsort((sel, -voxels[sel]))][:keep_largest])
    chosen = np.zeros(n + 1, bool)
    chosen[sel + 1] = True
    r = chosen[lab]
    labels = np.zeros((nz, ny, nx), np.int64)
    labels[crop] = lab
    full = np.zeros((nz, ny, nx), bool)
    full[crop] = r
    out = None
    if dst_contour is not None or label_channel is not None:
        out = np.zeros((nz, ny, nx, 4), f32) if dst is None else dst.copy()
        bits = out.view(np.uint32)
        if dst_contour is not None:
            cur = bits[..., dst_contour][crop]
            bits[..., dst_contour][crop] = {cr.REPLACE: np.where(r, cr.ONE, np.uint32(0)), cr.OR: np.where(r, cr.ONE, cur),
                                            cr.AND: np.where(r, cur, np.uint32(0)), cr.ANDNOT: np.where(r, np.uint32(0), cur)}[combine]
        if label_channel is not None:
            assert n <= cr.MAX_LABEL
            bits[..., label_channel][crop] = lab.astype(f32).view(np.uint32)
    lo, hi = cr.bounding_box(full)
    nodes, pairs = cr.run_counts(s, connectivity)
    result = (n, len(sel), int(s.sum()), int(r.sum()), int(voxels.max()) if n else 0, lo, hi)
    return dict(out=out, table=tab, selected=sel, result=result, counters=(int(s.size), nodes, pairs), labels=labels, r=full)


# ---- the label limit: 2^24 isolated voxels need 2^25 voxels ------------------------------------------------------------------------

LIMIT_SHAPE = (130, 512, 512)  # slices of 131 072 isolated voxels: 128 of them hold exactly 2^24


def isolated_labels(a):
    """The closed form for a set of isolated voxels (a FACES checkerboard): label = 1 + the voxel's rank among the set voxels in raster
    order, 0 outside; every component has one voxel, lo = first, hi = first + 1."""
    return np.where(a, np.cumsum(a.ravel(), dtype=np.int64).reshape(a.shape), 0)
