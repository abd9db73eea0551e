"""The numpy restatement of the gamma index (vr_volume_gamma, include/vr.h): every f32 operation the header names, in float32, the fused
steps through fma_ref.fma32; vectorised over the voxels of the box and over a chunk of the offset table, one loop over the chunks.
Volumes are (nz, ny, nx, 4) float32; spacing, boxes and offsets are (x, y, z).  Harness only."""
import numpy as np

from fma_ref import fma32

f32, u32, i64 = np.float32, np.uint32, np.int64
MAX_SUB, MAX_RADIUS = 4, 8
MAX_SPACING, MAX_REACH = 1 << 20, 1 << 24
GLOBAL, LOCAL = 0, 1
QNAN = 0x7FC00000
CELLS = 1 << 21  # candidates x voxels evaluated at a time


def bits_of(value):
    """The bits of a float as a descriptor's f32 field holds it."""
    return int(np.array([value], f32).view(u32)[0])


def radii(spacing, reach):
    return tuple(int(reach) // int(s) for s in spacing)


def valid(spacing, dta, reach, sub):
    """What the descriptor's own numbers must satisfy."""
    return (all(1 <= s <= MAX_SPACING for s in spacing) and 1 <= dta <= MAX_REACH and 1 <= reach <= MAX_REACH and 1 <= sub <= MAX_SUB
            and all(r <= MAX_RADIUS for r in radii(spacing, reach)))


def table(spacing, dta, reach, sub):
    """The admitted offsets in the order of the header: (o, D2n, c) with o an int64 (K, 3) array of (i, j, k), ascending D2n, ties by
    (k, j, i); D2n int64 (exact: below 2^53); c = (float)D2n * kc as float32."""
    lim = (int(reach) * int(sub)) ** 2
    ax = [np.arange(-(int(reach) * sub // int(s)), int(reach) * sub // int(s) + 1, dtype=i64) for s in spacing]
    k, j, i = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    d2 = (i * int(spacing[0])) ** 2 + (j * int(spacing[1])) ** 2 + (k * int(spacing[2])) ** 2
    keep = d2 <= lim
    i, j, k, d2 = i[keep], j[keep], k[keep], d2[keep]
    order = np.lexsort((i, j, k, d2))
    kc = f32(1.0 / (float(dta) * float(dta) * float(sub) * float(sub)))
    d2 = d2[order]
    c = d2.astype(np.float64).astype(f32) * kc  # (exact in f64, so one rounding to f32; then one product)
    return np.stack([i[order], j[order], k[order]], axis=1), d2, c.astype(f32)


def member(component):
    """vr_mask_distance's membership: != 0.0f -- NaN is in, -0.0f is out."""
    return component != 0


def field(R, E, roi, spacing, dta, reach, sub, mode, tol, cutoff, lo, hi, cut=False, chunk=None):
    """The search over the box lo .. hi of the (nz, ny, nx) float32 fields R and E (roi: a field or None).  Returns (G2 float32 with
    NaN where every g2 was NaN, skipped bool, candidates visited by evaluated voxels, K, asked), the first two and the last flat over
    the box, x fastest; asked = per voxel the table entries whose c was below its minimum (0 for a skipped voxel): where the cut stops
    it.
    cut: leave out, per voxel, the candidates whose c is not below the minimum as it stood before their chunk (chunk=1: the exact cut
    of the header).  The result must not depend on cut or chunk."""
    R, E = np.ascontiguousarray(R, f32), np.ascontiguousarray(E, f32)
    nz, ny, nx = R.shape
    n = (nx, ny, nz)
    o, _, c = table(spacing, dta, reach, sub)
    K = len(c)
    pz, py, px = [a.reshape(-1) for a in np.meshgrid(np.arange(lo[2], hi[2]), np.arange(lo[1], hi[1]), np.arange(lo[0], hi[0]), indexing="ij")]
    p = (px, py, pz)
    with np.errstate(all="ignore"):
        r = R[pz, py, px]
        T = np.full(r.shape, f32(tol), f32) if mode == GLOBAL else f32(tol) * r
        skipped = ~(r >= f32(cutoff)) | ~(np.isfinite(T) & (T > 0))
        if roi is not None:
            skipped |= ~member(np.asarray(roi, f32)[pz, py, px])
        inv_t = f32(1.0) / T
        G2 = np.full(r.shape, np.nan, f32)
        visited = 0
        asked = np.zeros(r.shape, np.int64)
        step = chunk if chunk else max(1, CELLS // max(1, r.size))
        for k0 in range(0, K if r.size else 0, step):
            ok = o[k0:k0 + step]
            ck = c[k0:k0 + step, None]
            m = np.floor_divide(ok, sub)
            f = ok - sub * m
            exists = np.ones((len(ok), r.size), bool)
            b = []
            for a in range(3):
                ba = p[a][None, :] + m[:, a, None]
                exists &= (ba >= 0) & (ba + (f[:, a, None] > 0) <= n[a] - 1)
                b.append(ba)
            t = [(f[:, a].astype(f32) / f32(sub))[:, None] for a in range(3)]
            fpos = [f[:, a, None] > 0 for a in range(3)]

            def at(dx, dy, dz):
                return E[np.clip(b[2] + dz, 0, nz - 1), np.clip(b[1] + dy, 0, ny - 1), np.clip(b[0] + dx, 0, nx - 1)]

            def lerp(u, v, ta, on):
                return np.where(on, fma32(ta, v - u, u), u) if on.any() else u

            def along_x(dy, dz):
                return lerp(at(0, dy, dz), at(1, dy, dz), t[0], fpos[0])

            def along_y(dz):
                return lerp(along_x(0, dz), along_x(1, dz), t[1], fpos[1])

            e = at(0, 0, 0) if sub == 1 else lerp(along_y(0), along_y(1), t[2], fpos[2])
            d = (e - r[None, :]) * inv_t[None, :]
            g2 = fma32(d, d, np.broadcast_to(ck, d.shape))
            take = exists & ~np.isnan(g2)
            asking = ~(ck >= G2[None, :])
            asked += (asking & ~skipped[None, :]).sum(axis=0)
            if cut:
                take &= asking
                visited += int((asking & exists & ~skipped[None, :]).sum())
            else:
                visited += int((exists & ~skipped[None, :]).sum())
            best = np.where(take, g2, f32(np.inf)).min(axis=0)
            G2 = np.where(take.any(axis=0) & (np.isnan(G2) | (best < G2)), best, G2)
    return G2, skipped, visited, K, asked


def gamma(ref, ev, before, ref_channel, eval_channel, dst_channel, spacing, dta, reach, sub=1, mode=GLOBAL, tol=1.0, cutoff=-np.inf,
          skip_bits=QNAN, roi=None, roi_contour=0, lo=None, hi=None, cut=False, chunk=None):
    """vr_volume_gamma.  ref, ev: the two dose volumes; before: the destination as it was (None: a fresh slot of zeros; may be ref or
    ev); roi: the ROI volume or None.  Returns (the destination after the call, (stored, evaluated, passed, nonfinite, bits of
    hi_value), (box voxels, evaluated, K))."""
    ref, ev = np.asarray(ref, f32), np.asarray(ev, f32)
    nz, ny, nx = ref.shape[:3]
    lo = (0, 0, 0) if lo is None else tuple(lo)
    hi = (nx, ny, nz) if hi is None else tuple(hi)
    out = np.zeros(ref.shape, f32) if before is None else np.array(before, f32, copy=True)
    shape = (hi[2] - lo[2], hi[1] - lo[1], hi[0] - lo[0])
    if shape[0] * shape[1] * shape[2] == 0:
        return out, (0, 0, 0, 0, 0), (0, 0, 0)
    G2, skipped, _, K, _ = field(ref[..., ref_channel], ev[..., eval_channel], None if roi is None else np.asarray(roi, f32)[..., roi_contour],
                                 spacing, dta, reach, sub, mode, tol, cutoff, lo, hi, cut, chunk)
    with np.errstate(all="ignore"):
        stored = np.sqrt(G2).astype(f32).view(u32).copy()
    stored[np.isnan(G2)] = QNAN
    stored[skipped] = u32(skip_bits)
    ev_mask = ~skipped
    passed = int((ev_mask & (G2 <= f32(1.0))).sum())
    nonfinite = ev_mask & ((stored & u32(0x7F800000)) == u32(0x7F800000))
    finite = ev_mask & ~nonfinite
    hi_bits = int(stored[finite].max()) if finite.any() else 0  # (stored values are +0 or positive: their bits order as they do)
    out.view(u32)[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0], dst_channel] = stored.reshape(shape)
    n_box, n_ev = int(stored.size), int(ev_mask.sum())
    return out, (n_box, n_ev, passed, int(nonfinite.sum()), hi_bits), (n_box, n_ev, K)
