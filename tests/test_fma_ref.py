"""fma_ref.fma32 -- the one fused multiply-add every fused float32 restatement goes through -- against exact rational arithmetic:
fractions.Fraction of the three float32 inputs, rounded to nearest even to float32 by the integer arithmetic below (subnormal results
and overflow to infinity included).  No tolerance: every result has the bits of the exact rounding; infinities and NaN behave as
IEEE fmaf does."""
import math
from fractions import Fraction

import numpy as np

import fma_ref as fr

f32 = np.float32
TWO = Fraction(2)


def bits(x):
    return np.asarray(x, f32).view(np.uint32)


def from_bits(b):
    return np.asarray(b, np.uint32).view(f32)


def round_f32(x):
    """Round-to-nearest-even of a nonzero Fraction to float32, as a Python float (exactly a float32 value, or +-inf)."""
    sign = -1.0 if x < 0 else 1.0
    x = abs(x)
    e = x.numerator.bit_length() - x.denominator.bit_length()  # 2^(e-1) < x < 2^(e+1)
    if x < TWO ** e:
        e -= 1
    assert TWO ** e <= x < TWO ** (e + 1)
    quantum = TWO ** (max(e, -126) - 23)  # the spacing of float32 at x (subnormals share the smallest normal's)
    n = x / quantum
    lo = n.numerator // n.denominator
    rem = n - lo
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and (lo & 1)):
        lo += 1
    r = lo * quantum
    if r >= TWO ** 128:
        return sign * math.inf
    return sign * float(r)  # (at most 24 significant bits, exponent within double's: exact)


def exact_fma(a, b, c):
    """IEEE fmaf(a, b, c) of three float32 values (Python floats), by exact arithmetic.  Returns a Python float."""
    if math.isnan(a) or math.isnan(b) or math.isnan(c):
        return math.nan
    if math.isinf(a) or math.isinf(b):
        if a == 0.0 or b == 0.0:
            return math.nan
        p = math.copysign(1.0, a) * math.copysign(1.0, b) * math.inf
        if math.isinf(c) and c != p:
            return math.nan
        return p
    if math.isinf(c):
        return c
    x = Fraction(a) * Fraction(b) + Fraction(c)
    if x != 0:
        return round_f32(x)
    # an exact zero: the sum of two zeros of one sign keeps it; every other exact zero is +0 (round to nearest)
    if a == 0.0 or b == 0.0:
        ps = math.copysign(1.0, a) * math.copysign(1.0, b)
        if ps == math.copysign(1.0, c):
            return math.copysign(0.0, c)
    return 0.0


def check(a, b, c, what):
    a, b, c = (np.ascontiguousarray(np.broadcast_to(np.asarray(x, f32), np.broadcast(a, b, c).shape)).ravel() for x in (a, b, c))
    got = fr.fma32(a, b, c)
    assert got.dtype == f32 and got.shape == a.shape
    want = np.array([exact_fma(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)], np.float64)
    nan = np.isnan(want)
    wb = bits(want.astype(f32))  # (already float32 values: the conversion is exact)
    bad = (np.isnan(got) != nan) | (~nan & (bits(got) != wb))
    print(what, len(a), "triples,", int(bad.sum()), "mismatches")
    k = np.nonzero(bad)[0][:5]
    assert not bad.any(), (what, [(float(a[i]).hex(), float(b[i]).hex(), float(c[i]).hex(), float(got[i]).hex(), float(want[i]).hex()) for i in k])


def random_f32(rng, n, emin, emax):
    """Random signs and 24-bit significands at exponents emin .. emax."""
    m = rng.integers(1 << 23, 1 << 24, size=n).astype(np.float64)
    e = rng.integers(emin, emax + 1, size=n).astype(np.float64)
    s = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    return (s * m * np.exp2(e - 23)).astype(f32)


def test_round_f32_itself():
    """The test's own rounding on values whose answer is known by construction."""
    assert round_f32(Fraction(1) + Fraction(1, 2 ** 24)) == 1.0  # a tie: to even
    assert round_f32(Fraction(1) + Fraction(3, 2 ** 24)) == 1.0 + 2.0 ** -22  # a tie: to even, upward
    assert round_f32(Fraction(1) + Fraction(1, 2 ** 24) + Fraction(1, 2 ** 200)) == 1.0 + 2.0 ** -23
    assert round_f32(Fraction(1, 2 ** 150)) == 0.0 and round_f32(Fraction(3, 2 ** 150)) == 2.0 ** -148  # subnormal ties
    assert round_f32(Fraction(1, 2 ** 150) + Fraction(1, 2 ** 300)) == 2.0 ** -149
    assert round_f32(-Fraction(5, 2 ** 150)) == -(2.0 ** -148)  # 2.5 quanta: a tie to the even 2
    assert round_f32(-Fraction(5, 2 ** 151)) == -(2.0 ** -149)  # 1.25 quanta
    top = Fraction(2 ** 128) - Fraction(2 ** 104)  # FLT_MAX
    assert round_f32(top) == float(top) and round_f32(top + Fraction(2 ** 103) - 1) == float(top)
    assert round_f32(top + Fraction(2 ** 103)) == math.inf and round_f32(-top - Fraction(2 ** 103)) == -math.inf
    for v in (1.0, -3.5, 2.0 ** -149, 2.0 ** -126, float(top), 1.0 + 2.0 ** -23):
        assert round_f32(Fraction(v)) == v


def test_random_triples():
    rng = np.random.default_rng(20240607)
    n = 12000
    # independent magnitudes
    check(random_f32(rng, n, -20, 20), random_f32(rng, n, -20, 20), random_f32(rng, n, -40, 40), "random")
    # the product cancels against c: c = -(a * b) rounded, a few ulps around it, and c = the product of neighbouring factors
    a, b = random_f32(rng, n, -8, 8), random_f32(rng, n, -8, 8)
    c = (-(a.astype(np.float64) * b.astype(np.float64))).astype(f32)
    c = from_bits((bits(c).astype(np.int64) + rng.integers(-3, 4, size=n)).astype(np.uint32))
    check(a, b, c, "cancelling")
    # the restatements' own shapes: a lerp (b - a) * t + a with t in [0, 1), a texture coordinate p * n - 0.5
    lo, hi, t = rng.random(n, dtype=f32), rng.random(n, dtype=f32), rng.random(n, dtype=f32)
    check(hi - lo, t, lo, "lerp")
    check(rng.random(n, dtype=f32), rng.choice([5, 7, 9, 13, 16, 20, 23, 64, 257], size=n).astype(f32), f32(-0.5), "coordinate")


def test_double_rounding_traps():
    """Exact values within half a float64 ulp of a float32 tie: a product and a sum each rounded to float64 would land on the tie and
    then go to even; the single rounding goes to the side of the tiny term."""
    rng = np.random.default_rng(7)
    n = 3000
    # (1) a * b is an odd 25-bit integer N -- a float32 tie -- and c is far below float64's last place of N
    x = rng.integers(1, 2048, size=n) * 2 + 1
    y = ((1 << 24) // x + 1) | 1
    y = np.where(x * y < (1 << 25), y, y - 2)
    N = x * y
    assert np.all((N >= 1 << 24) & (N < 1 << 25) & (N & 1 == 1))
    scale = np.exp2(rng.integers(-60, 60, size=n).astype(np.float64))
    tiny = np.exp2(-rng.integers(31, 90, size=n).astype(np.float64)) * np.where(rng.random(n) < 0.5, -1.0, 1.0)
    sign = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    a, b, c = (sign * x * scale).astype(f32), y.astype(f32), (tiny * scale).astype(f32)
    assert np.all(a.astype(np.float64) * b.astype(np.float64) == sign * N * scale) and np.all(c != 0)
    check(a, b, c, "tie + tiny")
    naive = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)
    assert np.any(bits(naive) != bits(fr.fma32(a, b, c))), "the traps do not trap a float64 sum"
    # (2) c = M * 2^47 and a * b = +-(2^46 - 1): one below half an ulp of c, 70 bits below c's top
    M = rng.integers(1 << 23, 1 << 24, size=n)
    sc = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    sp = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    scale = np.exp2(rng.integers(-80, 30, size=n).astype(np.float64))
    a = (sp * f32(2 ** 23 + 1) * scale).astype(f32)
    b = np.full(n, f32(2 ** 23 - 1))
    c = (sc * M * np.exp2(47.0) * scale).astype(f32)
    check(a, b, c, "just short of a tie")
    naive = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)
    assert np.any(bits(naive) != bits(fr.fma32(a, b, c))), "the traps do not trap a float64 sum"
    # (3) exact ties themselves: to even
    check((x * np.exp2(-10.0)).astype(f32), y.astype(f32), f32(0.0), "exact ties")
    check(f32(1.0), f32(2.0 ** -24), from_bits(bits(f32(1.0)) + np.arange(8, dtype=np.uint32)), "exact ties of a sum")


def test_subnormal_results_and_overflow():
    rng = np.random.default_rng(11)
    n = 6000
    # products around the subnormal range, alone and against subnormal / small normal c
    a, b = random_f32(rng, n, -80, -60), random_f32(rng, n, -80, -60)
    sub = from_bits(rng.integers(0, 1 << 23, size=n).astype(np.uint32) | (rng.integers(0, 2, size=n).astype(np.uint32) << 31))
    check(a, b, f32(0.0), "subnormal products")
    check(a, b, sub, "subnormal sums")
    check(a, b, random_f32(rng, n, -149 + 23, -120), "around the smallest normal")
    # exact ties between subnormals: k * 2^-150 with k odd, and one quantum of product beside them
    k = (rng.integers(0, 1 << 12, size=n) * 2 + 1).astype(f32)
    check(k * f32(2.0 ** -75), f32(2.0 ** -75), f32(0.0), "subnormal ties")
    check(k * f32(2.0 ** -75), f32(2.0 ** -75), np.where(rng.random(n) < 0.5, f32(2.0 ** -149), f32(-2.0 ** -149)), "subnormal ties + 1")
    check(k * f32(2.0 ** -75), f32(2.0 ** -75) * (f32(1.0) + f32(2.0 ** -23)), sub, "beside subnormal ties")
    # overflow: products and sums around FLT_MAX
    big = random_f32(rng, n, 60, 67)
    check(big, random_f32(rng, n, 60, 64), random_f32(rng, n, 100, 127), "around FLT_MAX")
    fmax = from_bits(np.uint32(0x7F7FFFFF))
    check(fmax, f32(1.0), from_bits(np.uint32(0x73000000) + np.arange(-4, 5).astype(np.uint32)), "FLT_MAX + half an ulp")
    check(f32(2.0 ** 64), f32(2.0 ** 64), np.array([-fmax, fmax, -(2.0 ** 127), 0.0], f32), "a product past FLT_MAX that c brings back or not")


def test_zeros_infinities_and_nan():
    z = np.array([0.0, -0.0], f32)
    vals = np.array([0.0, -0.0, 1.0, -1.0, 2.0 ** -149, -(2.0 ** -149), np.inf, -np.inf, np.nan, 3.0e38, -3.0e38], f32)
    A, B, Cc = (g.ravel() for g in np.meshgrid(vals, vals, vals, indexing="ij"))
    check(A, B, Cc, "special values")
    # the sign of an exact zero, spelled out
    for a, b, c, want in ((0.0, 1.0, 0.0, 0.0), (-0.0, 1.0, -0.0, -0.0), (-0.0, 1.0, 0.0, 0.0), (0.0, 1.0, -0.0, 0.0),
                          (-0.0, -1.0, -0.0, 0.0), (1.0, 1.0, -1.0, 0.0), (-1.0, 1.0, 1.0, 0.0), (2.0 ** -149, 2.0 ** -149, -0.0, 0.0),
                          (-(2.0 ** -149), 2.0 ** -149, 0.0, -0.0), (-(2.0 ** -149), 2.0 ** -149, -0.0, -0.0)):
        got = fr.fma32(f32(a), f32(b), f32(c))
        assert bits(got) == bits(f32(want)), (a, b, c, got)
    assert z.dtype == f32
    # fmaf's invalid operations and its propagation
    assert np.isnan(fr.fma32(f32(np.inf), f32(0.0), f32(1.0))) and np.isnan(fr.fma32(f32(np.inf), f32(1.0), f32(-np.inf)))
    assert np.isnan(fr.fma32(f32(0.0), f32(-np.inf), f32(np.nan))) and np.isnan(fr.fma32(f32(1.0), f32(1.0), f32(np.nan)))
    assert fr.fma32(f32(np.inf), f32(-2.0), f32(3.0)) == -np.inf and fr.fma32(f32(1.0), f32(2.0), f32(np.inf)) == np.inf
    assert fr.fma32(f32(np.inf), f32(2.0), f32(np.inf)) == np.inf and fr.fma32(f32(3.0e38), f32(3.0e38), f32(-np.inf)) == -np.inf


def test_mad_modes_and_slice_ref_share_it():
    """mad is a * b + c rounded twice or once, and slice_ref's fma32 is this one."""
    import slice_ref as slr
    assert slr.fma32 is fr.fma32
    rng = np.random.default_rng(3)
    a, b, c = rng.random(1000, dtype=f32), rng.random(1000, dtype=f32), rng.random(1000, dtype=f32) - f32(0.5)
    sep = fr.mad(a, b, c)
    assert sep.dtype == f32 and np.array_equal(bits(sep), bits((a * b).astype(f32) + c))
    fus = fr.mad(a, b, c, fused=True)
    assert np.array_equal(bits(fus), bits(fr.fma32(a, b, c))) and np.any(bits(fus) != bits(sep))
