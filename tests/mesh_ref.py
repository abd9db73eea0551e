"""A plain numpy / Python restatement of vr_volume_mesh's definition (include/vr.h): marching tetrahedra on the Kuhn split of every
cell.  Written from the definition, not from the kernels: loops over cells, a dict of edges, the orientation swap derived geometrically
with the vertices at a generic t.  Positions are computed in float32 exactly as the definition says (two subtractions, one division)."""
import itertools

import numpy as np

PERMS = list(itertools.permutations(range(3)))  # lexicographic: xyz, xzy, yxz, yzx, zxy, zyx
GENERIC_T = (0.3, 0.45, 0.6, 0.7, 0.35, 0.55)   # one per tetrahedron edge 01, 02, 03, 12, 13, 23: strictly inside, all different


def tetra(perm):
    """The four corner offsets q0 .. q3 of the tetrahedron of a permutation (a, b, c)."""
    q = [(0, 0, 0)]
    for a in perm:
        p = list(q[-1])
        p[a] += 1
        q.append(tuple(p))
    return q


def case_triangles(inside):
    """The triangles of a case as triples of corner pairs (i, j), i < j, before the swap."""
    ins = [i for i in range(4) if inside[i]]
    outs = [i for i in range(4) if not inside[i]]
    e = lambda a, b: (min(a, b), max(a, b))
    if len(ins) in (0, 4):
        return []
    if len(ins) == 2:
        (i, j), (k, l) = ins, outs
        return [(e(i, k), e(i, l), e(j, l)), (e(i, k), e(j, l), e(j, k))]
    i = ins[0] if len(ins) == 1 else outs[0]
    j, k, l = [x for x in range(4) if x != i]
    return [(e(i, j), e(i, k), e(i, l))]


def _swap_table():
    """swap[(tetrahedron, case)]: whether the last two indices are exchanged so that (p1 - p0) x (p2 - p0) points from the inside points
    toward the outside points, with every vertex at a generic t inside its edge.  Both triangles of a two-and-two case must agree."""
    names = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
    table = {}
    for T, perm in enumerate(PERMS):
        q = np.array(tetra(perm), float)
        for case in range(1, 15):
            inside = [(case >> i) & 1 for i in range(4)]
            cin = q[[i for i in range(4) if inside[i]]].mean(0)
            cout = q[[i for i in range(4) if not inside[i]]].mean(0)
            signs = []
            for tri in case_triangles(inside):
                p = [q[i] + GENERIC_T[names.index((i, j))] * (q[j] - q[i]) for i, j in tri]
                signs.append(float(np.dot(np.cross(p[1] - p[0], p[2] - p[0]), cout - cin)))
            assert all(abs(s) > 1e-9 for s in signs) and len({s > 0 for s in signs}) == 1, (T, case, signs)
            table[T, case] = signs[0] < 0
    return table


SWAP = _swap_table()


def extract(vol, level, cap, box_lo, box_hi, origin=(0, 0, 0)):
    """vol: float32 (nz, ny, nx) -- one component; origin: the voxel (x, y, z) of vol[0, 0, 0] where vol is a crop that holds the box
    (coordinates stay those of the whole volume).  Returns dict(vertices float32 (V, 3), triangles uint32 (T, 3), result = (V, T,
    inside, cells, lo, hi), edges = per vertex (p, m) with p in voxel coordinates)."""
    vol = np.asarray(vol, np.float32)
    level = np.float32(level)
    lo, hi = np.array(box_lo), np.array(box_hi)
    e = lo - cap                       # the first lattice point
    ln = hi - lo + 2 * cap             # lattice points per axis
    cn = ln - 1                        # cells per axis

    def real(p):
        return all(lo[a] <= p[a] < hi[a] for a in range(3))

    def value(p):
        return vol[p[2] - origin[2], p[1] - origin[1], p[0] - origin[0]]

    def inside(p):
        return bool(real(p) and value(p) >= level)

    n_inside = 0
    if (hi > lo).all():
        with np.errstate(invalid="ignore"):
            n_inside = int((vol[lo[2] - origin[2]:hi[2] - origin[2], lo[1] - origin[1]:hi[1] - origin[1], lo[0] - origin[0]:hi[0] - origin[0]] >= level).sum())
    if (hi <= lo).any() or (cn < 1).any():
        return dict(vertices=np.zeros((0, 3), np.float32), triangles=np.zeros((0, 3), np.uint32),
                    result=(0, 0, n_inside, 0, (0, 0, 0), (0, 0, 0)), edges=[])

    # pass 1: the triangles as edge keys, in cell order; the set of edges
    tris, edges = [], set()
    cells, clo, chi = 0, [None] * 3, [None] * 3
    for oz in range(cn[2]):
        for oy in range(cn[1]):
            for ox in range(cn[0]):
                o = (int(e[0]) + ox, int(e[1]) + oy, int(e[2]) + oz)
                before = len(tris)
                for T, perm in enumerate(PERMS):
                    q = [tuple(o[a] + s[a] for a in range(3)) for s in tetra(perm)]
                    ins = [inside(p) for p in q]
                    case = sum(int(b) << i for i, b in enumerate(ins))
                    for tri in case_triangles(ins):
                        keys = []
                        for i, j in tri:
                            d = tuple(q[j][a] - q[i][a] for a in range(3))
                            keys.append((q[i], d[0] + 2 * d[1] + 4 * d[2]))
                        if SWAP[T, case]:
                            keys[1], keys[2] = keys[2], keys[1]
                        tris.append(keys)
                        edges.update(keys)
                if len(tris) > before:
                    cells += 1
                    for a in range(3):
                        clo[a] = o[a] if clo[a] is None else min(clo[a], o[a])
                        chi[a] = o[a] + 1 if chi[a] is None else max(chi[a], o[a] + 1)

    # pass 2: number the edges in key order (raster index of p in the extended lattice, then m)
    def key(pm):
        p, m = pm
        l = [p[a] - e[a] for a in range(3)]
        return ((l[2] * int(ln[1]) + l[1]) * int(ln[0]) + l[0], m)

    order = sorted(edges, key=key)
    number = {pm: i for i, pm in enumerate(order)}
    verts = np.zeros((len(order), 3), np.float32)
    with np.errstate(all="ignore"):
        for i, (p, m) in enumerate(order):
            d = (m & 1, (m >> 1) & 1, m >> 2)
            b = tuple(p[a] + d[a] for a in range(3))
            if not real(p):
                t = np.float32(1)
            elif not real(b):
                t = np.float32(0)
            else:
                va, vb = value(p), value(b)
                t = np.float32(np.float32(level - va) / np.float32(vb - va))
                if not t >= 0:
                    t = np.float32(0)
                if t > 1:
                    t = np.float32(1)
            for a in range(3):
                verts[i, a] = np.float32(p[a]) + t if d[a] else np.float32(p[a])
    tri_idx = np.array([[number[k] for k in t] for t in tris], np.uint32).reshape(-1, 3)
    if cells == 0:
        clo, chi = [0] * 3, [0] * 3
    return dict(vertices=verts, triangles=tri_idx, result=(len(order), len(tris), n_inside, cells, tuple(int(x) for x in clo), tuple(int(x) for x in chi)), edges=order)


def counts(vol, level, cap, box_lo, box_hi):
    """(vertices, triangles, inside, cells) of a call, counted with whole-array numpy operations: the crossing lattice edges of the seven
    directions, one triangle per tetrahedron with 1 or 3 inside corners and two per tetrahedron with 2.  Independent of extract()."""
    lo, hi = np.array(box_lo), np.array(box_hi)
    if (hi <= lo).any():
        return 0, 0, 0, 0
    with np.errstate(invalid="ignore"):
        ins = np.asarray(vol, np.float32)[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]] >= np.float32(level)
    n_inside = int(ins.sum())
    if cap:
        ins = np.pad(ins, 1)
    if min(ins.shape) < 2:
        return 0, 0, n_inside, 0
    nz, ny, nx = ins.shape

    def corner(s):  # the corner s of every cell
        return ins[s[2]:nz - 1 + s[2], s[1]:ny - 1 + s[1], s[0]:nx - 1 + s[0]]

    n_v = 0
    for m in range(1, 8):
        d = (m & 1, (m >> 1) & 1, m >> 2)
        a = ins[:nz - d[2], :ny - d[1], :nx - d[0]]
        b = ins[d[2]:, d[1]:, d[0]:]
        n_v += int((a != b).sum())
    n_t, any_tri = 0, np.zeros((nz - 1, ny - 1, nx - 1), bool)
    for perm in PERMS:
        n = sum(corner(q).astype(np.int8) for q in tetra(perm))
        n_t += int(((n == 1) | (n == 3)).sum()) + 2 * int((n == 2).sum())
        any_tri |= (n > 0) & (n < 4)
    return n_v, n_t, n_inside, int(any_tri.sum())


# ---- properties ------------------------------------------------------------------------------------------------------------------------

def directed_edges(triangles):
    t = np.asarray(triangles, np.int64)
    return np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])


def edges_unique(triangles):
    """Every directed edge occurs at most once."""
    d = directed_edges(triangles)
    return len(np.unique(d, axis=0)) == len(d)


def is_closed(triangles):
    """Every directed edge occurs once and has its opposite."""
    d = directed_edges(triangles)
    if len(d) == 0:
        return True
    n = int(d.max()) + 1
    fwd, back = np.sort(d[:, 0] * n + d[:, 1]), np.sort(d[:, 1] * n + d[:, 0])
    return bool((fwd[1:] != fwd[:-1]).all() and np.array_equal(fwd, back))


def euler(n_vertices, triangles):
    d = directed_edges(triangles)
    und = np.unique(np.sort(d, axis=1), axis=0)
    return n_vertices - len(und) + len(triangles)


def signed_volume(vertices, triangles):
    """By the divergence theorem, in float64."""
    v = np.asarray(vertices, np.float64)
    t = np.asarray(triangles, np.int64)
    if len(t) == 0:
        return 0.0
    p0, p1, p2 = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    return float(np.einsum("ij,ij->i", p0, np.cross(p1, p2)).sum() / 6.0)
