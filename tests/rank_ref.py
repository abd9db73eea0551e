"""The numpy restatement of the rank filters (vr_volume_rank, include/vr.h): pad the keys with mode="edge" or "constant", take a
sliding_window_view, sort the keys of every window, take position k, un-key.  Nothing is computed: the result is one of the input bit
patterns.  Volumes are (nz, ny, nx, 4) float32; axes are named as the header names them (0 = x, 1 = y, 2 = z), radii and boxes are
(x, y, z).  Harness only."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

from filter_ref import key

f32, u32 = np.float32, np.uint32
MAX_RADIUS = 3
MIN, MEDIAN, MAX = 0, -1, -2
CLAMP, CONSTANT = 0, 1
CHUNK = 1 << 25  # keys sorted at a time


def bits_of(value):
    """The bits of a float as vr_rank_desc.border_value holds it (rounded to f32)."""
    return int(np.array([value], f32).view(u32)[0])


def unkey(k):
    """The f32 bit patterns of uint32 keys: the inverse of filter_ref.key."""
    k = np.asarray(k, u32)
    return np.where(k & u32(0x80000000), k & u32(0x7FFFFFFF), ~k).astype(u32)


def window(radii):
    return (2 * radii[0] + 1) * (2 * radii[1] + 1) * (2 * radii[2] + 1)


def resolve(rank, radii):
    """The position k a descriptor's rank means, or None for an invalid one."""
    n = window(radii)
    if rank == MEDIAN:
        return n // 2
    if rank == MAX:
        return n - 1
    return rank if 0 <= rank < n else None


def select(field, radii, rank, border=CLAMP, border_bits=0, lo=None, hi=None):
    """The selected bit patterns (uint32) of the box lo .. hi (x, y, z; the whole field by default) of a (nz, ny, nx) float32 field."""
    bits = np.ascontiguousarray(field, f32).view(u32)
    nz, ny, nx = bits.shape
    lo = (0, 0, 0) if lo is None else tuple(lo)
    hi = (nx, ny, nz) if hi is None else tuple(hi)
    rx, ry, rz = radii
    k = resolve(rank, radii)
    pad = ((rz, rz), (ry, ry), (rx, rx))
    keys = key(bits.view(f32))
    if border == CLAMP:
        p = np.pad(keys, pad, mode="edge")
    else:
        p = np.pad(keys, pad, mode="constant", constant_values=key(np.array([border_bits], u32).view(f32))[0])
    out = np.zeros((hi[2] - lo[2], hi[1] - lo[1], hi[0] - lo[0]), u32)
    if out.size == 0:
        return out
    n = window(radii)
    slab = max(1, CHUNK // (n * out.shape[1] * out.shape[2]))
    for z0 in range(0, out.shape[0], slab):  # (voxel z of the padded keys = z + rz: the window of box voxel z starts at padded z)
        z1 = min(out.shape[0], z0 + slab)
        sub = p[lo[2] + z0:lo[2] + z1 + 2 * rz, lo[1]:hi[1] + 2 * ry, lo[0]:hi[0] + 2 * rx]
        w = sliding_window_view(sub, (2 * rz + 1, 2 * ry + 1, 2 * rx + 1)).reshape(z1 - z0, out.shape[1], out.shape[2], n)
        out[z0:z1] = unkey(np.sort(w, axis=-1)[..., k])
    return out


def rank(src, before, src_channel, dst_channel, radii, rank=MEDIAN, border=CLAMP, border_bits=0, lo=None, hi=None):
    """vr_volume_rank.  src: the source volume; before: the destination as it was (None: a fresh slot of zeros; may be src itself).
    Returns (the destination after the call, (stored, nonfinite, changed, bits of lo_value, bits of hi_value), (box voxels, voxels of
    the box grown by the radii and clipped to the volume, k))."""
    src = np.asarray(src, f32)
    nz, ny, nx = src.shape[:3]
    lo = (0, 0, 0) if lo is None else tuple(lo)
    hi = (nx, ny, nz) if hi is None else tuple(hi)
    out = np.zeros(src.shape, f32) if before is None else np.array(before, f32, copy=True)
    box = (slice(lo[2], hi[2]), slice(lo[1], hi[1]), slice(lo[0], hi[0]))
    field = np.ascontiguousarray(src[..., src_channel])
    stored = select(field, radii, rank, border, border_bits, lo, hi)
    n_box = int(stored.size)
    if n_box == 0:
        return out, (0, 0, 0, 0, 0), (0, 0, 0)
    changed = int((stored != field.view(u32)[box]).sum())
    out.view(u32)[box + (dst_channel,)] = stored
    finite = (stored & u32(0x7F800000)) != u32(0x7F800000)
    lo_bits = hi_bits = 0
    if finite.any():
        flat = stored[finite]
        k = key(flat.view(f32))
        lo_bits, hi_bits = int(flat[np.argmin(k)]), int(flat[np.argmax(k)])
    read = 1
    for a, n_a in enumerate((nx, ny, nz)):
        read *= min(n_a, hi[a] + radii[a]) - max(0, lo[a] - radii[a])
    return out, (n_box, int((~finite).sum()), changed, lo_bits, hi_bits), (n_box, read, resolve(rank, radii))
