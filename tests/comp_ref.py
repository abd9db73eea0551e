"""Restatement of vr_mask_components (include/vr.h) that shares nothing with the kernels' union-find over runs: every voxel of S starts
with its own raster index, takes the minimum over its neighbours and jumps to the label of its label until nothing changes; a
component's label is then the index of its first voxel, and ranking those gives the definition's numbering.  Volumes are
float32[nz, ny, nx, 4]; boxes and voxels are (x, y, z) as in the descriptor.  No scipy."""
from itertools import product

import numpy as np

f32 = np.float32
FACES, ALL, PLANE_FACES, PLANE_ALL = 6, 26, 4, 8
REPLACE, OR, AND, ANDNOT = range(4)
MAX_KEEP, MAX_LABEL = 64, 1 << 24
ONE = np.array([1.0], f32).view(np.uint32)[0]
U64_MAX = (1 << 64) - 1


def member(component):
    """Membership of a float32 component: != 0.0f, so NaN is in and -0.0f is out."""
    return component != f32(0.0)


def offsets(connectivity):
    """The (dx, dy, dz) of a voxel's neighbours."""
    out = [d for d in product((-1, 0, 1), repeat=3) if d != (0, 0, 0)]
    if connectivity in (PLANE_FACES, PLANE_ALL):
        out = [d for d in out if d[2] == 0]
    if connectivity in (FACES, PLANE_FACES):
        out = [d for d in out if sum(1 for c in d if c) == 1]
    assert len(out) == connectivity
    return out


def shifted(shape, d):
    """Slices (dst, src) such that a[dst] and a[src] pair every voxel p with p + d, both inside `shape` (nz, ny, nx); d = (dx, dy, dz)."""
    dst, src = [], []
    for n, k in zip(shape, d[::-1]):
        dst.append(slice(max(0, -k), n - max(0, k)))
        src.append(slice(max(0, k), n - max(0, -k)))
    return tuple(dst), tuple(src)


def label(s, connectivity):
    """(labels int64[s.shape], n): 0 outside s, else 1 + the rank of the component's first voxel among all components' first voxels."""
    n = s.size
    if n == 0 or not s.any():
        return np.zeros(s.shape, np.int64), 0
    lab = np.where(s, np.arange(n, dtype=np.int64).reshape(s.shape), n)
    pairs = [shifted(s.shape, d) for d in offsets(connectivity)]
    while True:
        new = lab.copy()
        for dst, src in pairs:
            np.minimum(new[dst], lab[src], out=new[dst])
        new[~s] = n
        ext = np.append(new.ravel(), n)  # (ext[n] = n: outside stays outside)
        while True:
            jump = ext[ext]
            if np.array_equal(jump, ext):
                break
            ext = jump
        new = ext[:-1].reshape(s.shape)
        if np.array_equal(new, lab):
            break
        lab = new
    firsts = np.unique(lab[s])  # (sorted: the components' first voxels)
    out = np.zeros(s.shape, np.int64)
    out[s] = np.searchsorted(firsts, lab[s]) + 1
    return out, len(firsts)


def table(labels, n, box_lo):
    """[(voxels, lo, hi, first, faces)] of labels 1 .. n of a box's crop whose first voxel is box_lo."""
    if n == 0:
        return []
    shape = labels.shape
    z, y, x = np.nonzero(labels)
    c = labels[z, y, x] - 1
    voxels = np.bincount(c, minlength=n)
    lo = np.full((n, 3), 1 << 30, np.int64)
    hi = np.zeros((n, 3), np.int64)
    faces = np.zeros(n, np.int64)
    first = np.full(n, labels.size, np.int64)
    np.minimum.at(first, c, (z * shape[1] + y) * shape[2] + x)
    for a, (v, m) in enumerate(zip((x, y, z), shape[::-1])):
        np.minimum.at(lo[:, a], c, v)
        np.maximum.at(hi[:, a], c, v + 1)
        np.bitwise_or.at(faces, c, np.where(v == 0, 1 << (2 * a), 0) | np.where(v == m - 1, 2 << (2 * a), 0))
    out = []
    for i in range(n):
        f = int(first[i])
        fx, fy, fz = f % shape[2], f // shape[2] % shape[1], f // (shape[2] * shape[1])
        out.append((int(voxels[i]), tuple(int(lo[i, a]) + box_lo[a] for a in range(3)), tuple(int(hi[i, a]) + box_lo[a] for a in range(3)),
                    (fx + box_lo[0], fy + box_lo[1], fz + box_lo[2]), int(faces[i])))
    return out


def table_arrays(labels, n, box_lo):
    """table() as five arrays, for masks with a million components: (voxels int64[n], lo int64[n, 3], hi int64[n, 3], first int64[n, 3],
    faces int64[n]), the triples (x, y, z).  No loop over components: the set voxels are sorted by label, stably, so each component's
    voxels stand together in raster order, its first in front, and every column is one reduction over those segments."""
    shape = labels.shape
    if n == 0:
        return np.zeros(0, np.int64), np.zeros((0, 3), np.int64), np.zeros((0, 3), np.int64), np.zeros((0, 3), np.int64), np.zeros(0, np.int64)
    flat = np.flatnonzero(labels)
    c = labels.ravel()[flat] - 1
    order = np.argsort(c, kind="stable")
    voxels = np.bincount(c, minlength=n).astype(np.int64)
    assert voxels.min() > 0
    starts = np.concatenate(([0], np.cumsum(voxels)[:-1]))
    zyx = np.unravel_index(flat[order], shape)
    lo, hi, first = np.zeros((n, 3), np.int64), np.zeros((n, 3), np.int64), np.zeros((n, 3), np.int64)
    faces = np.zeros(n, np.int64)
    for a, (v, m) in enumerate(zip(zyx[::-1], shape[::-1])):
        v = v.astype(np.int64)
        lo[:, a] = np.minimum.reduceat(v, starts) + box_lo[a]
        hi[:, a] = np.maximum.reduceat(v, starts) + 1 + box_lo[a]
        first[:, a] = v[starts] + box_lo[a]
        faces |= np.bitwise_or.reduceat(np.where(v == 0, 1 << (2 * a), 0) | np.where(v == m - 1, 2 << (2 * a), 0), starts)
    return voxels, lo, hi, first, faces


def select(tab, min_voxels=1, max_voxels=U64_MAX, reject_faces=0, keep_largest=0):
    """The 0-based numbers of the selected components, ascending."""
    ok = [i for i, t in enumerate(tab) if min_voxels <= t[0] <= max_voxels and not (t[4] & reject_faces)]
    if keep_largest:
        ok = sorted(sorted(ok, key=lambda i: (-tab[i][0], i))[:keep_largest])
    return ok


def run_counts(s, connectivity):
    """(nodes, pairs): the maximal runs along x of s, and the pairs (run, run that touches it in an earlier row the connectivity names).
    Runs lengthened by one voxel at their far end stay disjoint within a row, and two runs touch under a reach of 1 exactly when the
    lengthened ones overlap; two runs overlap exactly where both are set and one of them starts."""
    if s.size == 0:
        return 0, 0
    e = connectivity in (ALL, PLANE_ALL)
    wide = np.zeros(s.shape[:2] + (s.shape[2] + 1,), bool)
    wide[..., :-1] = s
    start = wide.copy()
    start[..., 1:] &= ~wide[..., :-1]
    if e:
        wide[..., 1:] |= wide[..., :-1].copy()
    rows = {FACES: [(-1, 0), (0, -1)], ALL: [(-1, 0), (-1, -1), (0, -1), (1, -1)], PLANE_FACES: [(-1, 0)], PLANE_ALL: [(-1, 0)]}[connectivity]
    pairs = 0
    for dy, dz in rows:
        dst, src = shifted(wide.shape, (0, dy, dz))
        pairs += int((wide[dst] & wide[src] & (start[dst] | start[src])).sum())
    return int(start.sum()), pairs


def bounding_box(r):
    """(lo, hi) of r as (x, y, z) triples, half open; zeros when r is empty."""
    if not r.any():
        return (0, 0, 0), (0, 0, 0)
    z, y, x = np.nonzero(r)
    return (int(x.min()), int(y.min()), int(z.min())), (int(x.max()) + 1, int(y.max()) + 1, int(z.max()) + 1)


def components(src, dst, src_contour, background, connectivity, box_lo, box_hi, min_voxels=1, max_voxels=U64_MAX, reject_faces=0,
               keep_largest=0, dst_contour=None, combine=REPLACE, label_channel=None):
    """One vr_mask_components.  src: the source slot's voxels; dst: the written slot's before the call (None: an empty slot or no slot
    written; pass src itself for a call that writes its source slot); dst_contour / label_channel None: not asked for.  Returns a dict:
    out (the written slot's voxels after the call, None if none is written), table, selected (0-based numbers), result (n_components,
    n_selected, |S|, |R|, largest, lo, hi), counters (voxels of the box, nodes, pairs), labels and r (whole-volume arrays)."""
    nz, ny, nx = src.shape[:3]
    (x0, y0, z0), (x1, y1, z1) = box_lo, box_hi
    crop = (slice(z0, z1), slice(y0, y1), slice(x0, x1))
    s = member(src[..., src_contour])[crop]
    if background:
        s = ~s
    lab, n = label(s, connectivity)
    tab = table(lab, n, box_lo)
    sel = select(tab, min_voxels, max_voxels, reject_faces, keep_largest)
    r = np.isin(lab, np.array(sel, np.int64) + 1)
    labels = np.zeros((nz, ny, nx), np.int64)
    labels[crop] = lab
    full = np.zeros((nz, ny, nx), bool)
    full[crop] = r
    out = None
    if dst_contour is not None or label_channel is not None:
        out = np.zeros((nz, ny, nx, 4), f32) if dst is None else dst.copy()
        bits = out.view(np.uint32)
        if dst_contour is not None:
            comp = bits[..., dst_contour]
            cur = comp[crop]
            new = {REPLACE: np.where(r, ONE, np.uint32(0)), OR: np.where(r, ONE, cur), AND: np.where(r, cur, np.uint32(0)),
                   ANDNOT: np.where(r, np.uint32(0), cur)}[combine]
            comp[crop] = new
        if label_channel is not None:
            assert n <= MAX_LABEL
            bits[..., label_channel][crop] = lab.astype(f32).view(np.uint32)
    lo, hi = bounding_box(full)
    nodes, pairs = run_counts(s, connectivity)
    result = (n, len(sel), int(s.sum()), int(r.sum()), max([t[0] for t in tab], default=0), lo, hi)
    return dict(out=out, table=tab, selected=sel, result=result, counters=(int(s.size), nodes, pairs), labels=labels, r=full)
