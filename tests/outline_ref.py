"""The restatement of contour tracing (vr_mask_outlines, include/vr.h) in numpy, formulated as the kernels work: the two corner masks per
64-bit vertex word from the packed voxel rows, the scan of their counts that numbers the corner nodes, the link of every node to the next
corner along its edge, pointer doubling over the predecessors for leader and rank, and the emit.  tests/test_outline.py pins it against a
sequential crack walker, against raster_ref and against closed forms."""
import numpy as np

SPLIT, JOIN = 0, 1
MAX_COORD, MAX_SPACING = 1 << 29, 1 << 20
BIG = 1 << 40


def member(component):
    """The membership rule of the mask tools: != 0.0f (NaN is in, -0 is out)."""
    return np.asarray(component, np.float32) != np.float32(0.0)


def members(vol):
    """(nz, ny, nx, 4) float32 voxels -> boolean (4, nz, ny, nx)."""
    return np.stack([member(vol[..., k]) for k in range(4)])


def _popcount(w):
    return np.unpackbits(np.ascontiguousarray(w).view(np.uint8), bitorder="little").reshape(w.shape + (64,)).sum(-1).astype(np.int64)


def _bits(w):
    """uint64 words (..., n) -> their bits as booleans (..., 64 n), bit p of word q at 64 q + p."""
    return np.unpackbits(np.ascontiguousarray(w).view(np.uint8), axis=-1, bitorder="little").astype(bool)


def corner_words(s, lo, hi):
    """The vertex words of one contour.  s: boolean (slices, ny, nx), already cut to the box; lo, hi: the box's rows.  Returns
    (sw, se, nw, ne, one, two) as uint64 (slices, hi - lo + 1, nx // 64 + 1): the four voxels around each vertex, the vertices with one
    corner, with two."""
    nzb, ny, nx = s.shape
    vwx = nx // 64 + 1
    padded = np.zeros((nzb, ny + 2, vwx * 64), bool)  # row y + 1 = voxel row y; the rows and bits beyond the volume are out
    padded[:, 1:ny + 1, :nx] = s
    words = np.packbits(padded, axis=-1, bitorder="little").view("<u8")  # (slices, ny + 2, vwx)
    a, b = words[:, lo:hi + 1], words[:, lo + 1:hi + 2]                    # vertex row j: voxel rows j - 1 and j

    def up(w):  # shifted up by one bit, with the carry of the word before
        carry = np.zeros_like(w)
        carry[..., 1:] = w[..., :-1] >> np.uint64(63)
        return (w << np.uint64(1)) | carry

    sw, se, nw, ne = up(a), a, up(b), b
    one = sw ^ se ^ nw ^ ne
    two = (sw & ne & ~se & ~nw) | (se & nw & ~sw & ~ne)
    return sw, se, nw, ne, one, two


def trace(m, contours, connect, box_lo, box_hi, origin=(0, 0), spacing=(1, 1), offset=(0, 0), plain=False):
    """One vr_mask_outlines.  m: boolean (4, nz, ny, nx), the members of each contour.  Returns a dict: points int32 (N, 2), polygons
    [(first, count, slice, contour)], result (as OutlinesResult.as_tuple), rounds (the doubling rounds launched), longest (the points of
    the longest polygon)."""
    _, nz, ny, nx = m.shape
    kmap = [k for k in range(4) if (contours >> k) & 1]
    (x0, y0, z0), (x1, y1, z1) = box_lo, box_hi
    empty = dict(points=np.zeros((0, 2), np.int32), polygons=[], result=(0, 0, (0,) * 4, (0,) * 4, (0,) * 4), rounds=0, longest=0)
    if x1 <= x0 or y1 <= y0 or z1 <= z0:
        return empty
    nc, nzb, rows, vwx = len(kmap), z1 - z0, y1 - y0 + 1, nx // 64 + 1
    V = vwx * 64
    inbox = np.zeros((nzb, ny, nx), bool)
    inbox[:, y0:y1, x0:x1] = True
    quads = [corner_words(m[k, z0:z1] & inbox, y0, y1) for k in kmap]
    sw, se, nw, ne, one, two = (np.stack([q[i] for q in quads]).reshape(nc * nzb * rows, vwx) for i in range(6))
    # the scan over the words numbers the nodes: contour, slice, vertex row, word; inside a word by bit, a saddle's two by direction
    counts = _popcount(one) + 2 * _popcount(two)
    base = np.cumsum(counts.ravel()) - counts.ravel()
    n = int(counts.sum())
    if n == 0:
        return empty
    assert n <= 0x7fffffff
    one_b, two_b = _bits(one), _bits(two)
    per_vertex = one_b.astype(np.int64) + 2 * two_b
    below = np.cumsum(per_vertex.reshape(-1, 64), axis=1) - per_vertex.reshape(-1, 64)  # the nodes of the word below each bit
    node0 = (base[:, None] + below).ravel()                                                # the first node of every vertex
    vert = np.repeat(np.arange(per_vertex.size), per_vertex.ravel())                       # node -> vertex (row * V + i)
    ids = np.arange(n)
    second = ids - node0[vert]
    r, i = vert // V, vert % V
    jr = r % rows
    zr = (r // rows) % nzb
    c = r // (rows * nzb)
    j = y0 + jr
    # the edges that leave a vertex, the voxel on their left: 0 = +x, 1 = +y, 2 = -x, 3 = -y
    bsw, bse, bnw, bne = (_bits(w).ravel() for w in (sw, se, nw, ne))
    leave = np.stack([bne & ~bse, bnw & ~bne, bsw & ~bnw, bse & ~bsw])
    first_dir, last_dir = np.argmax(leave, axis=0), 3 - np.argmax(leave[::-1], axis=0)
    d = np.where(second == 1, last_dir[vert], first_dir[vert])
    # the next corner along the edge: the next set bit of one | two in the row, or the same bit row by row
    anyb = one_b | two_b
    col = np.arange(V)[None, :]
    right = np.full((anyb.shape[0], V + 1), BIG)
    right[:, :V] = np.minimum.accumulate(np.where(anyb, col, BIG)[:, ::-1], axis=1)[:, ::-1]
    left = np.full((anyb.shape[0], V + 1), -1)
    left[:, 1:] = np.maximum.accumulate(np.where(anyb, col, -1), axis=1)
    cube = anyb.reshape(nc * nzb, rows, V)
    row = np.arange(rows)[None, :, None]
    upw = np.full((nc * nzb, rows + 1, V), BIG)
    upw[:, :rows] = np.minimum.accumulate(np.where(cube, row, BIG)[:, ::-1], axis=1)[:, ::-1]
    down = np.full((nc * nzb, rows + 1, V), -1)
    down[:, 1:] = np.maximum.accumulate(np.where(cube, row, -1), axis=1)
    cz = r // rows
    i2 = np.where(d == 0, right[r, i + 1], np.where(d == 2, left[r, i], i))
    jr2 = np.where(d == 1, upw[cz, jr + 1, i], np.where(d == 3, down[cz, jr, i], jr))
    assert (i2 >= 0).all() and (i2 < V).all() and (jr2 >= 0).all() and (jr2 < rows).all()
    vert2 = (cz * rows + jr2) * V + i2
    saddle = two_b.ravel()[vert2]
    assert (saddle | one_b.ravel()[vert2]).all()
    d2 = np.where(saddle, (d + (3 if connect == JOIN else 1)) & 3, first_dir[vert2])
    succ = node0[vert2] + np.where(saddle, d2 >> 1, 0)
    pred = np.full(n, -1, np.int64)
    pred[succ] = ids
    assert (pred >= 0).all() and len(np.unique(succ)) == n  # every node has one successor and one predecessor
    j2 = y0 + jr2
    cross = i * j2 - i2 * j
    area2 = [0] * 4
    for q, k in enumerate(kmap):
        area2[k] = int(cross[c == q].sum())
    px = origin[0] - offset[0] + i * spacing[0]
    py = origin[1] - offset[1] + j * spacing[1]
    assert max(np.abs(px).max(), np.abs(py).max()) <= MAX_COORD
    # leader and rank by pointer doubling: (the smallest node of the backward window, its offset, the node one window back)
    fixed = 0
    while (1 << fixed) < n:
        fixed += 1
    low, off, jump, rounds = ids.copy(), np.zeros(n, np.int64), pred.copy(), 0
    for rnd in range(fixed):
        better = low[jump] < low
        low, off, jump = np.where(better, low[jump], low), np.where(better, off[jump] + (1 << rnd), off), jump[jump]
        rounds += 1
        if not plain and not better.any():
            break
    # emit
    leader = low == ids
    pidx = np.cumsum(leader) - leader
    count = off[pred[leader]] + 1
    first = np.cumsum(count) - count
    points = np.zeros((n, 2), np.int32)
    where = first[pidx[low]] + off
    assert len(np.unique(where)) == n
    points[where, 0], points[where, 1] = px, py
    kk = np.asarray(kmap)[c]
    polygons = [(int(f), int(cn), int(z), int(k)) for f, cn, z, k in zip(first, count, z0 + zr[leader], kk[leader])]
    polygons_of, points_of = [0] * 4, [0] * 4
    for k in kmap:
        polygons_of[k] = int((kk[leader] == k).sum())
        points_of[k] = int((kk == k).sum())
    return dict(points=points, polygons=polygons, result=(n, len(polygons), tuple(polygons_of), tuple(points_of), tuple(area2)), rounds=rounds,
                longest=int(count.max()))
