"""The numpy restatement of the separable filters (vr_volume_filter and vr_filter_gaussian, include/vr.h): the Gaussian weights in
float64, and the passes with one rounded f32 product for the first tap and fma_ref.fma32 for every further tap, in ascending tap order,
vectorised over the field.  Volumes are (nz, ny, nx, 4) float32; axes are named as the header names them (0 = x, 1 = y, 2 = z), boxes
are (x, y, z).  Harness only."""
import numpy as np

from fma_ref import fma32

f32 = np.float32
MAX_RADIUS = 32
CLAMP, CONSTANT = 0, 1


def radius(sigma, truncate=4.0):
    return int(truncate * sigma + 0.5)


def gaussian64(sigma, order=0, truncate=4.0):
    """The 2 r + 1 weights in float64, before the rounding to f32: the header's formula, term by term."""
    r = radius(sigma, truncate)
    phi = [float(np.exp(np.float64(-0.5 * x * x / (sigma * sigma)))) for x in range(r + 1)]
    tail = 0.0
    for x in range(1, r + 1):
        tail += phi[x]
    s = phi[0] + 2.0 * tail
    w = np.zeros(2 * r + 1, np.float64)
    for x in range(r + 1):
        if order == 0:
            w[r + x] = w[r - x] = phi[x] / s
        else:
            w[r + x] = (x / (sigma * sigma)) * phi[x] / s
            w[r - x] = -w[r + x]
    if order == 1:
        w[r] = 0.0
    return w


def gaussian(sigma, order=0, truncate=4.0):
    """The weights as vr_filter_gaussian stores them: gaussian64 rounded to f32 (the centre of order 1 is +0.0f)."""
    w = gaussian64(sigma, order, truncate).astype(f32)
    if order == 1:
        w[len(w) // 2] = f32(0.0)
    return w


def correlate(field, w, axis, border=CLAMP, border_value=0.0):
    """One pass along `axis` (0 = x: the last numpy axis of a (nz, ny, nx) field) with weights w[0 .. 2r]: indices beyond a face read the
    face's value (CLAMP) or border_value (CONSTANT)."""
    field, w = np.asarray(field, f32), np.asarray(w, f32)
    r = len(w) // 2
    ax = field.ndim - 1 - axis
    n = field.shape[ax]
    pad = [(0, 0)] * field.ndim
    pad[ax] = (r, r)
    p = np.pad(field, pad, mode="edge") if border == CLAMP else np.pad(field, pad, mode="constant", constant_values=f32(border_value))

    def tap(t):
        idx = [slice(None)] * field.ndim
        idx[ax] = slice(t, t + n)
        return p[tuple(idx)]

    with np.errstate(all="ignore"):
        acc = w[0] * tap(0)  # (f32 x f32: one rounded product)
        for t in range(1, 2 * r + 1):
            acc = fma32(w[t], tap(t), acc)
    return acc.astype(f32)


def key(a):
    """uint32 keys that order f32 bit patterns as their values, -0.0f below +0.0f."""
    b = np.ascontiguousarray(a, f32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def regions(n, lo, hi, radii, has_pass):
    """Per pass, in order, the voxels it computes: the box grown on every later axis that has a pass by that axis' radius, clipped to
    the volume n = (nx, ny, nz)."""
    axes = [a for a in range(3) if has_pass[a]]
    out = []
    for k, _ in enumerate(axes):
        v = 1
        for a in range(3):
            l, h = lo[a], hi[a]
            if a in axes[k + 1:]:
                l, h = max(0, l - radii[a]), min(n[a], h + radii[a])
            v *= h - l
        out.append(v)
    return out


def filter(src, before, src_channel, dst_channel, taps, border=CLAMP, border_value=0.0, lo=None, hi=None):
    """vr_volume_filter.  src: the source volume; before: the destination as it was (None: a fresh slot of zeros; may be src itself);
    taps: per axis x, y, z the weights or None.  Returns (the destination after the call, (stored, nonfinite, bits of lo_value, bits of
    hi_value), (box voxels, computed values, passes))."""
    src = np.asarray(src, f32)
    nz, ny, nx = src.shape[:3]
    lo = (0, 0, 0) if lo is None else tuple(lo)
    hi = (nx, ny, nz) if hi is None else tuple(hi)
    field = np.ascontiguousarray(src[..., src_channel])
    for a in range(3):
        if taps[a] is not None:
            field = correlate(field, taps[a], a, border, border_value)
    out = np.zeros(src.shape, f32) if before is None else np.array(before, f32, copy=True)
    box = (slice(lo[2], hi[2]), slice(lo[1], hi[1]), slice(lo[0], hi[0]))
    stored = field[box]
    out.view(np.uint32)[box + (dst_channel,)] = stored.view(np.uint32)  # (bits: a NaN's payload survives the copy of no pass)
    n_box = int(stored.size)
    if n_box == 0:
        return out, (0, 0, 0, 0), (0, 0, 0)
    finite = np.isfinite(stored)
    lo_bits = hi_bits = 0
    if finite.any():
        k = key(stored[finite])
        flat = stored[finite].view(np.uint32)
        lo_bits, hi_bits = int(flat[np.argmin(k)]), int(flat[np.argmax(k)])
    has = [t is not None for t in taps]
    radii = [0 if t is None else len(t) // 2 for t in taps]
    computed = regions((nx, ny, nz), lo, hi, radii, has)
    return out, (n_box, int((~finite).sum()), lo_bits, hi_bits), (n_box, int(sum(computed)), len(computed))
