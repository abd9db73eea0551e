"""Cases of the gamma index at the edges of its kernels (csrc/vr_gamma.h), shared by tests/test_gamma.py (the conditions each case must
meet, on the CPU, through gamma_ref alone) and tests/test_gamma_gpu.py (the kernels against the restatement): shapes around the tile of
32 x 8 x 4 outputs with halos longer than the axes, rods of 65535 voxels, one lane that needs the whole table beside 63 that need one
entry, minima that tie with a later entry's c bit for bit, and a random sweep.  Volumes are (nz, ny, nx, 4) float32; spacing, boxes and
offsets are (x, y, z).  Harness only."""
import numpy as np

import gamma_ref as gr
import index_edges_cases as ie
import resample_cases as rc
from fma_ref import fma32

f32, u32, i64 = np.float32, np.uint32, np.int64
TILE = (32, 8, 4)  # kGammaTX, kGammaTY, kGammaTZ


def doses(shape, seed, shift=1.03, noise=0.4):
    """Two dose volumes around 20 with every other component arbitrary: the evaluated one the reference scaled and perturbed."""
    rng = np.random.default_rng(seed)
    ref, ev = rc.volume(shape, seed), rc.volume(shape, seed + 1)
    ref[..., 3] = (20.0 + 5.0 * rng.normal(0.0, 1.0, shape)).astype(f32)
    ev[..., 3] = (ref[..., 3] * f32(shift) + rng.normal(0.0, noise, shape)).astype(f32)
    return ref, ev


def halo(spacing, reach, sub):
    """The halo of a tile per axis, as vr_api_gamma.h sets it."""
    return tuple(int(reach) // int(s) + (1 if sub > 1 else 0) for s in spacing)


def steps(spacing, dta, reach, sub):
    """(m, f) per table entry: the base-voxel step floor(o / sub) and the sub-step, int64 (K, 3)."""
    o = gr.table(spacing, dta, reach, sub)[0]
    m = np.floor_divide(o, sub)
    return m, o - sub * m


def missing(shape, spacing, dta, reach, sub, lo=None, hi=None):
    """Per voxel of the box (flat, x fastest): the table entries that are no candidate there, beyond a face or without their upper
    corner."""
    nx, ny, nz = rc.n_of(shape)
    lo, hi = lo or (0, 0, 0), hi or (nx, ny, nz)
    m, f = steps(spacing, dta, reach, sub)
    out = []
    for a, n in enumerate((nx, ny, nz)):
        b = np.arange(lo[a], hi[a])[None, :] + m[:, a, None]
        out.append((b >= 0) & (b + (f[:, a, None] > 0) <= n - 1))  # (K, extent of the box along a)
    exists = out[2][:, :, None, None] & out[1][:, None, :, None] & out[0][:, None, None, :]
    return (~exists).sum(axis=0).reshape(-1)


# ---- a. shapes around the tile --------------------------------------------------------------------------------------------------------
# One below, at and one above 32 along x, 8 along y and 4 along z; axes of 1; two tiles and a tail on every axis at once.
EDGE_SHAPES = [(2, 3, 31), (2, 3, 32), (2, 3, 33), (2, 7, 5), (2, 8, 5), (2, 9, 5), (3, 3, 5), (4, 3, 5), (5, 3, 5), (1, 1, 1), (1, 1, 40),
               (1, 12, 1), (6, 1, 1), (9, 17, 65)]
EDGE = dict(spacing=(1000, 1000, 1000), dta=2000, reach=2000)  # K = 33 at sub 1, 257 at sub 2; the halo 2 and 3
# At sub 2 the halo's extra voxel is read only where reach * sub / spacing is no multiple of sub: with a reach of 2.5 voxels the offsets
# of +-5 half steps have the base voxel -3 and the upper corner +3.  With EDGE no entry of the sub 2 table reaches the third voxel.
EDGE_HALF = dict(spacing=(1000, 1000, 1000), dta=2000, reach=2500)
EDGE_RUNS = [(1, EDGE), (2, EDGE), (2, EDGE_HALF)]  # (sub, the table) of every edge shape
EDGE_TOL = 0.6
EDGE_BOX = ((30, 6, 2), (35, 10, 6))  # of (9, 17, 65): across a tile edge on every axis


def edge_doses(shape):
    """E is R scaled by 1.2 with noise of 2.0: the dose term at the voxel itself is several tolerances, so that the least g2 lies at a
    distant candidate in many voxels.  A notch along the longest axis makes voxel (0, 0, 0) depend on the halo's last voxel at sub 2: R
    = 80 there, E = 400 and -240 at the second and third voxel on, so that e = fmaf(0.5f, -640, 400) = 80 exactly at 2.5 voxels, the
    offset of five half steps (c = 1.5625, gamma = 1.25), and nowhere else within reach; and E = 80 at the far end of that line, one
    voxel from voxel (0, 0, 0) for a read that wraps round."""
    ref, ev = doses(shape, 300 + shape[0] + 10 * shape[1] + 100 * shape[2], shift=1.2, noise=2.0)
    if max(shape) >= 5:
        line = [0, 0, 0]
        at = lambda i: tuple(line[:int(np.argmax(shape))] + [i] + line[int(np.argmax(shape)) + 1:]) + (3,)
        ref[at(0)], ev[at(0)], ev[at(2)], ev[at(3)], ev[at(max(shape) - 1)] = f32(80.0), f32(400.0), f32(400.0), f32(-240.0), f32(80.0)
    return ref, ev


def search(R, E, spacing, dta, reach, sub, tol, beyond="drop", staged=None):
    """The stored bits of VR_GAMMA_GLOBAL over the whole (nz, ny, nx) fields, entry by entry, written apart from gamma_ref.field so that
    it can be made wrong on purpose.  beyond: what a position beyond a face is -- "drop": no candidate (the header); "clamp": the face's
    voxel; "wrap": the voxel as many steps from the opposite face.  staged: per axis the voxels on either side of the voxel that may be
    read (None: all); an entry whose base voxel or upper corner lies further out is dropped."""
    R, E = np.ascontiguousarray(R, f32), np.ascontiguousarray(E, f32)
    nz, ny, nx = R.shape
    n = (nx, ny, nz)
    c = gr.table(spacing, dta, reach, sub)[2]
    m, f = steps(spacing, dta, reach, sub)
    z, y, x = np.indices(R.shape)
    p = (x, y, z)
    inv_t = f32(1.0) / f32(tol)
    t = [f32(v) / f32(sub) for v in range(sub)]
    G2 = np.full(R.shape, np.nan, f32)

    def pick(v, a):
        return v % n[a] if beyond == "wrap" else np.clip(v, 0, n[a] - 1)

    with np.errstate(all="ignore"):
        for k in range(len(c)):
            mk, fk = m[k], f[k]
            if staged is not None and any(max(abs(int(mk[a])), abs(int(mk[a]) + (1 if fk[a] else 0))) > staged[a] for a in range(3)):
                continue
            b = [p[a] + int(mk[a]) for a in range(3)]
            exists = np.ones(R.shape, bool)
            if beyond == "drop":
                for a in range(3):
                    exists &= (b[a] >= 0) & (b[a] + (1 if fk[a] else 0) <= n[a] - 1)

            def at(dx, dy, dz):
                return E[pick(b[2] + dz, 2), pick(b[1] + dy, 1), pick(b[0] + dx, 0)]

            def along_x(dy, dz):
                u = at(0, dy, dz)
                return fma32(t[fk[0]], at(1, dy, dz) - u, u) if fk[0] else u

            def along_y(dz):
                u = along_x(0, dz)
                return fma32(t[fk[1]], along_x(1, dz) - u, u) if fk[1] else u

            u = along_y(0)
            e = fma32(t[fk[2]], along_y(1) - u, u) if fk[2] else u
            d = (e - R) * inv_t
            g2 = fma32(d, d, np.full(R.shape, c[k], f32))
            take = exists & ~np.isnan(g2) & (np.isnan(G2) | (g2 < G2))
            G2 = np.where(take, g2, G2)
        stored = np.sqrt(G2).astype(f32).view(u32).copy()
    stored[np.isnan(G2)] = gr.QNAN
    return stored


def short_halo(spacing, reach, sub):
    """The second mutant's staging: one voxel less than the halo on every axis."""
    return tuple(h - 1 for h in halo(spacing, reach, sub))


# ---- b. rods ----------------------------------------------------------------------------------------------------------------------------
RODS = ie.RODS  # (nx, ny, nz)
ROD_TOL = 0.6


def rod_doses(n):
    return doses((n[2], n[1], n[0]), 71)


def rod_far_box(n):
    return tuple(max(0, v - 70) for v in n), tuple(n)


# ---- c. the lone asker ------------------------------------------------------------------------------------------------------------------
# One lane of a wavefront asks for every entry of the table, the 63 others (and every other lane of the launch) for entry 0 alone.
LONE_SHAPE = (8, 16, 64)
LONE = dict(spacing=(1000, 1000, 3000), dta=3000, reach=6000)  # K = 293
LONE_SUB2 = dict(spacing=(1000, 1000, 3000), dta=3000, reach=3000)
LONE_TOL = 0.6
LONE_AT = (5, 9, 40)   # (z, y, x)
LONE_BOX = ((3, 2, 1), (64, 16, 8))  # 61 x 14 x 7 outputs: the last tile is 29 x 6 x 3
LONE_AT_BOX = (7, 15, 63)  # its lane 28 of row 5 and third output: beside lanes beyond the box along x, y and z
OUTLIER = f32(500.0)


def lone_cases():
    """name -> (ref, ev, where the outlier is (z, y, x), box or None).  "r": E = R but for one voxel of R; "e": R constant, one voxel of
    E; "r_box": as "r", the outlier in the last partial tile of a box off the tile origin."""
    ref, _ = doses(LONE_SHAPE, 3)
    out = {}
    for name, at in (("r", LONE_AT), ("r_box", LONE_AT_BOX)):
        r, e = ref.copy(), ref.copy()
        r[at + (3,)] = OUTLIER
        out[name] = (r, e, at, LONE_BOX if name == "r_box" else None)
    r = ref.copy()
    r[..., 3] = f32(20.0)
    e = r.copy()
    e[LONE_AT + (3,)] = OUTLIER
    out["e"] = (r, e, LONE_AT, None)
    return out


def asked_of(ref, ev, p, sub, tol, box=None):
    """(asked per voxel of the box as a (z, y, x) array, K, the bits of G2 likewise) of the exact cut."""
    shape = ref.shape[:3]
    lo, hi = box if box else ((0, 0, 0), rc.n_of(shape))
    G2, skipped, _, K, asked = gr.field(ref[..., 3], ev[..., 3], None, p["spacing"], p["dta"], p["reach"], sub, gr.GLOBAL, tol, -np.inf, lo, hi,
                                        cut=True, chunk=1)
    ext = (hi[2] - lo[2], hi[1] - lo[1], hi[0] - lo[0])
    assert not skipped.any()
    return asked.reshape(ext), K, G2.view(u32).reshape(ext)


# ---- d. exact ties ----------------------------------------------------------------------------------------------------------------------
# Integer doses, a tolerance of 1/2 and a distance to agreement of one unit: d = 2 (e - r) is an integer (at sub 2 every lerp of integers
# by 0 or 1/2 is a multiple of 1/8 -- d * d a multiple of 1/16), c = D2n / (dta sub)^2 an integer: every g2 is exact, and a minimum that
# equals the next entry's c bit for bit is common.
TIE_SHAPE = (9, 17, 65)
TIE_TOL = 0.5
TIES = {1: dict(spacing=(1, 1, 1), dta=1, reach=3), 2: dict(spacing=(2, 2, 2), dta=1, reach=6)}  # K = 123 and 925


def tie_doses():
    rng = np.random.default_rng(7)
    ref, ev = np.zeros(TIE_SHAPE + (4,), f32), np.zeros(TIE_SHAPE + (4,), f32)
    ref[..., 3] = rng.integers(0, 6, TIE_SHAPE).astype(f32)
    ev[..., 3] = rng.integers(0, 6, TIE_SHAPE).astype(f32)
    return ref, ev


def tie_share(ref, ev, sub):
    """(the share of voxels whose final G2 equals, bit for bit, the c of the entry at which they stop asking; the most entries a voxel
    asks for; K)."""
    asked, K, G2 = asked_of(ref, ev, TIES[sub], sub, TIE_TOL)
    c = gr.table(sub=sub, **TIES[sub])[2]
    stop = np.minimum(asked, K - 1)
    tie = (asked < K) & (c.view(u32)[stop] == G2)
    return float(tie.mean()), int(asked.max()), K


# ---- e. the sweep -----------------------------------------------------------------------------------------------------------------------
SPACINGS = (500, 977, 1000, 2500, 3000)
ROI_KINDS = ("none", "eval", "dst", "third")          # no ROI / in E's slot / in the destination's own slot and channel / a third slot
DST_KINDS = ("fresh", "separate", "on_ref", "on_eval")
PAYLOAD = 0x7FA12345
MAX_CELLS = 1 << 24  # box voxels x K


def table_size(spacing, reach, sub):
    lim = (reach * sub) ** 2
    ax = [np.arange(-(reach * sub // s), reach * sub // s + 1, dtype=i64) * s for s in spacing]
    return int(((ax[2] ** 2)[:, None, None] + (ax[1] ** 2)[None, :, None] + (ax[0] ** 2)[None, None, :] <= lim).sum())


def sweep(n=40, seed=7):
    rng = np.random.default_rng(seed)
    cases = []
    for i in range(n):
        shape = (int(rng.integers(1, 13)), int(rng.integers(1, 21)), int(rng.integers(1, 81)))
        nx, ny, nz = rc.n_of(shape)
        spacing = tuple(int(rng.choice(SPACINGS)) for _ in range(3))
        wide = bool(rng.random() < 0.125)
        radius = int(rng.integers(4, 9)) if wide else int(rng.integers(0, 4))
        # the finest axis has that radius: so many of its voxels and a part of one more
        reach = max(1, min(spacing) * radius + int(rng.integers(0, min(spacing))))
        dta = int(rng.choice([500, 1000, 2000, 3000, 4500]))
        sub = int(rng.integers(1, 5))
        mode = int(rng.integers(2))
        box = ("whole", "whole", "random", "random", "random", "random")[int(rng.integers(6))] if rng.random() < 0.95 else "empty"
        lo = [int(rng.integers(0, m)) for m in (nx, ny, nz)]
        hi = [int(rng.integers(l + 1, m + 1)) for l, m in zip(lo, (nx, ny, nz))]
        if box == "whole":
            lo, hi = [0, 0, 0], [nx, ny, nz]
        if box == "empty":
            a = int(rng.integers(3))
            hi[a] = lo[a]
        K = table_size(spacing, reach, sub)
        voxels = lambda: int(np.prod([h - l for l, h in zip(lo, hi)]))
        while voxels() * K > MAX_CELLS or (wide and voxels() > 64):
            a = int(np.argmax([h - l for l, h in zip(lo, hi)]))  # halve the longest side
            hi[a] = lo[a] + (hi[a] - lo[a]) // 2
            box = "random"
        roi, dst = ROI_KINDS[int(rng.integers(4))], DST_KINDS[int(rng.integers(4))]
        if roi == "dst" and dst == "fresh":  # (an ROI needs a filled slot)
            dst = "separate"
        cr, ce, cd = (int(rng.integers(4)) for _ in range(3))
        if ce == cr and roi == "third" and dst in ("fresh", "separate"):  # (both doses share a slot there)
            ce = (cr + 1) % 4
        cases.append(dict(shape=shape, seed=2000 + 3 * i, spacing=spacing, dta=dta, reach=reach, sub=sub, mode=mode, K=K,
                          tol=float(rng.choice([0.03, 0.05])) if mode else float(rng.choice([0.3, 0.6, 1.5])),
                          cutoff=float(rng.choice([-np.inf, 15.0, 19.0])), skip_bits=int(rng.choice([gr.QNAN, PAYLOAD, 0xFFFFFFFF, 0])),
                          roi=roi, dst=dst, box=box, lo=tuple(lo), hi=tuple(hi), chans=(cr, ce, cd), roi_contour=int(rng.integers(4)),
                          hostile=bool(rng.random() < 0.33), flavour=int(rng.integers(2)), layout=int(rng.choice([0, 1, 3]))))
    return cases


def sweep_volumes(case):
    """(slots, chans, roi, vols) of a sweep case: slots = the slots of R, E and the destination, chans their channels, roi = (slot,
    contour) or (-1, 0), vols = {slot: voxels before the call}, without the destination's slot where that is fresh.  A context has
    three slots: with the ROI in a third slot and a destination of its own, both doses lie in slot 0."""
    shape, seed = case["shape"], case["seed"]
    rng = np.random.default_rng(seed + 2)
    cr, ce, cd = case["chans"]
    if case["hostile"]:
        ref, ev = rc.hostile(shape, seed), rc.hostile(shape, seed + 1)
    else:
        ref, ev = doses(shape, seed, shift=1.05, noise=1.0)
        ref[..., cr], ev[..., ce] = ref[..., 3].copy(), ev[..., 3].copy()
    own = case["dst"] in ("fresh", "separate")
    if case["roi"] == "third" and own:
        ref[..., ce] = ev[..., ce]
        sr, se, vols = 0, 0, {0: ref}
    else:
        sr, se, vols = 0, 1, {0: ref, 1: ev}
    sd = {"fresh": 2, "separate": 2, "on_ref": sr, "on_eval": se}[case["dst"]]
    cd = {"on_ref": cr, "on_eval": ce}.get(case["dst"], cd)
    if case["dst"] == "separate":
        vols[2] = rc.arbitrary_bits(shape, seed + 5)
    roi = (-1, 0)
    if case["roi"] != "none":
        m = np.where(rng.random(shape) < 0.6, f32(1.0), f32(0.0)).astype(f32)
        m[rng.random(shape) < 0.1] = f32(np.nan)
        m[rng.random(shape) < 0.1] = f32(-0.0)
        if case["roi"] == "eval":
            roi = (se, (ce + 1 + case["roi_contour"] % 3) % 4)  # (a contour beside E's channel)
        elif case["roi"] == "dst":
            roi = (sd, cd)  # the contour the result overwrites
        else:
            roi = (1 if own else 2, case["roi_contour"])
            vols[roi[0]] = rc.volume(shape, seed + 7)
        if not (case["roi"] == "dst" and not own):  # (on a dose the dose itself is the ROI: in where it is not 0)
            vols[roi[0]][..., roi[1]] = m
    return (sr, se, sd), (cr, ce, cd), roi, vols
