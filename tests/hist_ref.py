"""numpy restatement of the device histogram (vr_histogram, include/vr.h): the rules and nothing of the kernel's structure.
A volume is float32[nz, ny, nx, 4] (x fastest), a descriptor anything with vr_hist_desc's fields (capi.HistDesc)."""
import numpy as np

f32 = np.float32
ROWS, MAX_BINS = 5, 65536
CLAMP, DROP = 0, 1
I32_MIN, I32_MAX = -(2 ** 31), 2 ** 31 - 1


def to_i32(t):
    """The normative f32 -> i32 conversion: truncation toward zero, saturating, NaN -> 0.  int64 values."""
    t = np.asarray(t, dtype=f32)
    out = np.zeros(t.shape, dtype=np.int64)
    fin = np.isfinite(t)
    # (every finite f32 and both limits are exact in float64: truncate and saturate there, then convert)
    out[fin] = np.clip(np.trunc(t[fin].astype(np.float64)), float(I32_MIN), float(I32_MAX)).astype(np.int64)
    out[np.isposinf(t)] = I32_MAX
    out[np.isneginf(t)] = I32_MIN
    return out


def index(v, scale):
    """i = i32(v * scale), the product one f32 multiply."""
    with np.errstate(all="ignore"):
        return to_i32(np.asarray(v, dtype=f32) * f32(scale))


def selects(m):
    """The mask rule: a component selects iff it is != 0.0f -- NaN selects, -0 does not."""
    return np.asarray(m, dtype=f32) != f32(0.0)


def histogram(desc, volume, mask=None):
    """(counts uint64[5, bins], rows = [(voxels, dropped)] * 5, voxels of the box)."""
    lo, hi = [int(x) for x in desc.lo], [int(x) for x in desc.hi]
    bins, rows_bits = int(desc.bins), int(desc.rows)
    box = (slice(lo[2], hi[2]), slice(lo[1], hi[1]), slice(lo[0], hi[0]))
    i = index(volume[box + (int(desc.channel),)], desc.scale).ravel()
    if int(desc.out_of_range) == CLAMP:
        counted = np.ones(i.shape, dtype=bool)
        b = np.clip(i, 0, bins - 1)
    else:
        counted = (i >= 0) & (i < bins)
        b = i
    counts = np.zeros((ROWS, bins), dtype=np.uint64)
    rows = [(0, 0)] * ROWS
    for r in range(ROWS):
        if not (rows_bits >> r) & 1:
            continue
        sel = np.ones(i.shape, dtype=bool) if r == 0 else selects(mask[box + (r - 1,)]).ravel()
        counts[r] = np.bincount(b[sel & counted], minlength=bins).astype(np.uint64)
        rows[r] = (int(sel.sum()), int((sel & ~counted).sum()))
    return counts, rows, int(i.size)
