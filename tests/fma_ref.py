"""The fused multiply-add of the float32 restatements (VR_ARITH_FUSED of include/vr.h): fma32 is the correctly rounded f32
a * b + c, mad the `a * b + c` of either arithmetic mode.  Proven against exact rational arithmetic by tests/test_fma_ref.py; shared
by proj_ref (and through it iso_ref, shadow_ref, surf_ref, bound_ref) and slice_ref.  Harness only."""
import numpy as np

f32 = np.float32


def fma32(a, b, c):
    """Correctly rounded f32 a * b + c: the product is exact in f64, the f64 sum is rounded to odd (TwoSum tells whether it was
    inexact and to which side), and rounding that to f32 is then the single rounding of the exact value."""
    a, b, c = (np.asarray(x, f32).astype(np.float64) for x in np.broadcast_arrays(a, b, c))
    with np.errstate(all="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)
        fix = np.isfinite(s) & np.isfinite(e) & (e != 0.0) & ((s.view(np.int64) & 1) == 0)
        toward = np.where(e > 0.0, np.inf, -np.inf)
        s = np.where(fix, np.nextafter(s, toward), s)
        return s.astype(f32)


def mad(a, b, c, fused=False):
    """a * b + c: product and sum rounded separately, or (fused) rounded once."""
    if fused:
        return fma32(a, b, c)
    with np.errstate(all="ignore"):
        return a * b + c
