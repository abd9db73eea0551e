"""The hull of the active bricks on the CPU (csrc/vr_hull.h through tests/hull_driver, compiled with g++): which steps of a ray the
skipping kernels may leave out.

A frame comparison on the device sees a plane that is too tight only if a test scene happens to have a ray there, so the rule is
swept here: restricted to the three axes steps_near_hull is the box function it replaced, bit for bit (the driver keeps that
function as the reference); with all 13 directions no position of a ray that lies in a brick of the set may fall outside [k0, k1]
-- the positions are the kernels' own (f32 rounded additions, brick_of in either arithmetic mode), the planes come from the numpy
restatement (tests/hull_ref.py) through the host's hull_bounds.  Only positions inside [0, 1]^3 count: a march samples no other
(IsInSampleCoords), and brick_of clamps those beyond the volume into its edge bricks.  No case is skipped or tolerated."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import hull_ref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(HERE, "_build")
CSRC = os.path.join(ROOT, "volumerendering_amd", "csrc")
f32 = np.float32
HALF = 0.125  # kBrickHalf: half a cell of a brick of four


def build_driver() -> str:
    os.makedirs(OUT, exist_ok=True)
    so = os.path.join(OUT, "libhull_driver.so")
    srcs = [os.path.join(HERE, "hull_driver", "hull_driver.cpp"), os.path.join(CSRC, "vr_hull.h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        tmp = so + f".{os.getpid()}.tmp"
        subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Werror", "-ffp-contract=off", "-I", CSRC, "-o", tmp, srcs[0]],
                       check=True)
        os.replace(tmp, so)
    return so


def ptr(a, t):
    return a.ctypes.data_as(C.POINTER(t))


@pytest.fixture(scope="module")
def lib():
    L = C.CDLL(build_driver())
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int)
    L.hd_dirs.argtypes = [ip]
    L.hd_bounds.argtypes = [C.c_int, ip, ip, fp, C.c_float, fp]
    L.hd_steps.argtypes = [fp, fp, fp, fp, C.c_int, C.c_int, ip]
    L.hd_steps_box.argtypes = [fp, fp, fp, C.c_int, ip]
    L.hd_axes_sweep.argtypes = [C.c_uint, C.c_int, ip]
    L.hd_walk.restype = C.c_longlong
    L.hd_walk.argtypes = [C.POINTER(C.c_ubyte), ip, fp, C.c_float, fp, C.c_int, fp, fp, ip, C.c_int, ip, ip]
    return L


def bounds(lib, kind, lo=None, hi=None, bs=(1.0, 1.0, 1.0)):
    out = np.zeros(26, dtype=f32)
    lo = np.asarray(lo if lo is not None else [0] * 13, dtype=np.int32)
    hi = np.asarray(hi if hi is not None else [0] * 13, dtype=np.int32)
    lib.hd_bounds(kind, ptr(lo, C.c_int), ptr(hi, C.c_int), ptr(np.asarray(bs, dtype=f32), C.c_float), HALF, ptr(out, C.c_float))
    return out


def steps(lib, p, s, bs, planes, n_steps, axes_only=False):
    k = np.zeros(2, dtype=np.int32)
    lib.hd_steps(ptr(np.asarray(p, dtype=f32), C.c_float), ptr(np.asarray(s, dtype=f32), C.c_float), ptr(np.asarray(bs, dtype=f32), C.c_float),
                 ptr(planes, C.c_float), n_steps, int(axes_only), ptr(k, C.c_int))
    return int(k[0]), int(k[1])


def walk(lib, active, bs, planes, p, s, n_steps, fused):
    """(violations, k[n, 2], steps in the set[n]) of hd_walk for the rays p[n, 3], s[n, 3], n_steps[n]."""
    bnz, bny, bnx = active.shape
    st = np.ascontiguousarray(active, dtype=np.uint8)
    bn = np.array([bnx, bny, bnz], dtype=np.int32)
    p, s = np.ascontiguousarray(p, dtype=f32), np.ascontiguousarray(s, dtype=f32)
    n_steps = np.ascontiguousarray(n_steps, dtype=np.int32)
    k, hits = np.zeros((len(p), 2), dtype=np.int32), np.zeros(len(p), dtype=np.int32)
    bad = lib.hd_walk(ptr(st, C.c_ubyte), ptr(bn, C.c_int), ptr(np.asarray(bs, dtype=f32), C.c_float), HALF, ptr(planes, C.c_float), len(p),
                      ptr(p, C.c_float), ptr(s, C.c_float), ptr(n_steps, C.c_int), int(fused), ptr(k, C.c_int), ptr(hits, C.c_int))
    return int(bad), k, hits


def test_directions_are_the_restatements(lib):
    d = np.zeros(39, dtype=np.int32)
    assert lib.hd_dirs(ptr(d, C.c_int)) == 13
    assert np.array_equal(d.reshape(13, 3), hull_ref.DIRS)


def test_axes_alone_are_the_box_function_bit_for_bit(lib):
    cases = np.zeros(3, dtype=np.int32)
    n = 400000
    assert lib.hd_axes_sweep(20240517, n, ptr(cases, C.c_int)) == 0
    zero_step, nan, miss = (int(c) for c in cases)
    assert zero_step > n // 20 and nan > n // 20 and n // 20 < miss < n - n // 20, (zero_step, nan, miss)


def test_axis_planes_are_the_box_of_before(lib):
    """hull_bounds' first three pairs: (box_lo - 1 + 1/8) / bs and (box_hi + 2 + 1/8) / bs evaluated in double, rounded once."""
    rng = np.random.default_rng(5)
    for _ in range(200):
        bs = (rng.integers(1, 65536, 3) / 4.0).astype(f32)
        lo = rng.integers(0, 100, 13).astype(np.int32)
        hi = lo + rng.integers(0, 100, 13).astype(np.int32)
        pl = bounds(lib, 0, lo, hi, bs)
        for a in range(3):
            assert pl[a] == f32((float(lo[a]) - 1.0 + HALF) / float(bs[a]))
            assert pl[13 + a] == f32((float(hi[a]) + 2.0 + HALF) / float(bs[a]))


def test_diagonal_planes_hold_the_bricks_and_their_margin(lib):
    """Diagonal pair d bounds g . p = n . q + 1/8 sum(n): [lo - #neg - |n|_1, hi + #pos + |n|_1] + 1/8 sum(n), never rounded inward."""
    lo = np.array([3, 4, 5, 7, -9, 8, -2, 9, -1, 12, 2, 4, -6], dtype=np.int32)
    hi = lo + np.arange(13, dtype=np.int32)
    pl = bounds(lib, 0, lo, hi, (24.0, 16.0, 20.0))
    for d in range(3, 13):
        n = hull_ref.DIRS[d]
        neg, pos, l1, sm = int((n < 0).sum()), int((n > 0).sum()), int(np.abs(n).sum()), int(n.sum())
        assert float(pl[d]) <= lo[d] - neg - l1 + HALF * sm and float(pl[d]) > lo[d] - neg - l1 + HALF * sm - 1e-3
        assert float(pl[13 + d]) >= hi[d] + pos + l1 + HALF * sm and float(pl[13 + d]) < hi[d] + pos + l1 + HALF * sm + 1e-3


# ---- soundness ---------------------------------------------------------------------------------------------------------------------

GRIDS = {  # name: voxels per axis (bricks of four: bs = n / 4, bn = ceil(n / 4))
    "cube64": (64, 64, 64),       # bs equal and a power of two: rays exactly parallel to a diagonal plane exist
    "box96x64x80": (96, 64, 80),
    "odd90x61x77": (90, 61, 77),  # bs not whole: the last brick of an axis is cut
}


def brick_sets(bn, rng):
    bnx, bny, bnz = bn
    z, y, x = np.meshgrid(np.arange(bnz), np.arange(bny), np.arange(bnx), indexing="ij")
    sets = {}
    one = np.zeros((bnz, bny, bnx), dtype=bool)
    one[rng.integers(bnz), rng.integers(bny), rng.integers(bnx)] = True
    sets["single"] = one
    corners = np.zeros_like(one)
    corners[::bnz - 1, ::bny - 1, ::bnx - 1] = True
    sets["corners"] = corners
    sets["one_corner"] = (x == bnx - 1) & (y == 0) & (z == bnz - 1)
    sets["oblique_slab"] = np.abs(x + y - z - (bnx + bny - bnz) // 2) <= 0
    sets["oblique_slab2"] = (np.abs(x - y + z - bnx // 2) <= 0) & (x > 2)
    faces = np.zeros_like(one)
    for _ in range(6):
        b = [rng.integers(bnx), rng.integers(bny), rng.integers(bnz)]
        a = rng.integers(3)
        b[a] = 0 if rng.integers(2) else bn[a] - 1
        faces[b[2], b[1], b[0]] = True
    sets["faces"] = faces
    sets["ellipsoid"] = ((x + 0.5 - bnx / 2) / (0.42 * bnx)) ** 2 + ((y + 0.5 - bny / 2) / (0.35 * bny)) ** 2 + ((z + 0.5 - bnz / 2) / (0.45 * bnz)) ** 2 <= 1
    sets["random"] = rng.random(one.shape) < 3.0 / one.size
    sets["random"][rng.integers(bnz), rng.integers(bny), rng.integers(bnx)] = True
    return sets


def rays_at(active, bs, rng, n, exact_parallel):
    """n rays aimed at bricks of the set from anywhere around the volume: plain ones, rays with one or two step components exactly 0,
    rays exactly parallel to a diagonal plane (a cube grid: bs equal, a power of two), 4 000-step rays and rays that graze."""
    bz, by, bx = np.nonzero(active)
    bs = np.asarray(bs, dtype=np.float64)
    p, s, ns = [], [], []
    for i in range(n):
        j = rng.integers(len(bx))
        target = (np.array([bx[j], by[j], bz[j]]) + rng.random(3) * 1.4 - 0.2 + HALF) / bs
        a = rng.random(3) * 1.6 - 0.3
        kind = i % 8
        if kind == 1:
            a[rng.integers(3)] = target[rng.integers(3)]  # (usually another axis: a plain ray; the same one: a zero component)
        if kind == 2:
            ax = rng.integers(3)
            a[ax] = target[ax]
        if kind == 3:
            ax = rng.integers(3)
            keep = a[ax]
            a = target.copy()
            a[ax] = keep
        n_steps = int(rng.choice([200, 886, 4000])) if kind != 4 else 4000
        step = ((target - a) * (1.0 + rng.random()) / n_steps).astype(f32)
        if kind in (2, 3):
            assert (step == 0).any()
        if exact_parallel and kind == 5:
            step[1] = step[0] if rng.integers(2) else -step[0]          # n = (1, -1, 0) / (1, 1, 0)
        if exact_parallel and kind == 6:
            step[2] = -f32(step[0] + step[1]) if rng.integers(2) else f32(step[0] + step[1])   # n = (1, 1, 1) / (1, 1, -1)
        if kind == 7:  # a ray that grazes: a start a brick or two beside the set, a direction along one of its planes' normals' complements
            step[rng.integers(3)] *= f32(1e-4)
        p.append(a.astype(f32))
        s.append(step)
        ns.append(n_steps)
    return np.array(p), np.array(s), np.array(ns)


@pytest.mark.parametrize("grid", sorted(GRIDS))
def test_no_position_in_the_set_is_left_out(lib, grid):
    nvox = GRIDS[grid]
    bs = tuple(v / 4.0 for v in nvox)
    bn = tuple((v + 3) // 4 for v in nvox)
    rng = np.random.default_rng(sum(nvox))
    total_hits, rays_hit, misses, parallel = 0, 0, 0, 0
    for name, active in brick_sets(bn, rng).items():
        lo, hi = hull_ref.planes_of_set(active)
        planes = bounds(lib, 0, lo, hi, bs)
        p, s, ns = rays_at(active, bs, rng, 320, grid == "cube64")
        v = (s.astype(np.float64) * np.asarray(bs)) @ hull_ref.DIRS.T.astype(np.float64)
        parallel += int(((v[:, 3:] == 0) & (np.abs(s).sum(1) > 0)[:, None]).any(1).sum())
        for fused in (0, 1):
            bad, k, hits = walk(lib, active, bs, planes, p, s, ns, fused)
            assert bad == 0, (grid, name, fused, bad)
            # a reported miss: no step of the ray lies in the set
            assert not ((k[:, 1] < 0) & (hits > 0)).any(), (grid, name, fused)
            total_hits += int(hits.sum())
            rays_hit += int((hits > 0).sum())
            misses += int((k[:, 1] < 0).sum())
    # the sweep is not vacuous: most rays meet the set, some are pruned altogether, some run exactly along a diagonal plane
    assert rays_hit > 2000 and total_hits > 20000 and misses > 20, (rays_hit, total_hits, misses)
    if grid == "cube64":
        assert parallel > 100, parallel


def test_nan_excludes_nothing(lib):
    active = np.zeros((16, 16, 16), dtype=bool)
    active[5, 6, 7] = True
    bs = (16.0, 16.0, 16.0)
    planes = bounds(lib, 0, *hull_ref.planes_of_set(active), bs)
    nan = float("nan")
    assert steps(lib, (nan, nan, nan), (0.001, 0.001, 0.001), bs, planes, 886) == (0, 889)
    assert steps(lib, (0.1, 0.1, 0.1), (nan, nan, nan), bs, planes, 886) == (0, 889)
    # one NaN component: that axis and every diagonal through it say nothing, the others still hold
    rng = np.random.default_rng(9)
    p, s, ns = rays_at(active, bs, rng, 64, True)
    p[::2, 0] = nan
    s[1::2, 2] = nan
    for fused in (0, 1):
        bad, k, hits = walk(lib, active, bs, planes, p, s, ns, fused)
        assert bad == 0


def test_hull_prunes_more_crossing_rays_than_its_box(lib):
    """Tightness sanity: an ellipsoid of bricks, orthographic rays across the volume from random directions."""
    bn, bs = (24, 16, 20), (24.0, 16.0, 20.0)
    active = brick_sets(bn, np.random.default_rng(1))["ellipsoid"]
    planes = bounds(lib, 0, *hull_ref.planes_of_set(active), bs)
    rng = np.random.default_rng(2)
    pruned_hull = pruned_box = crossing = 0
    for _ in range(40):
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        u = np.cross(d, [0.3, 0.5, 0.8])
        u /= np.linalg.norm(u)
        w = np.cross(d, u)
        for _ in range(50):
            c = 0.5 + u * (rng.random() - 0.5) * 1.6 + w * (rng.random() - 0.5) * 1.6
            a, step = (c - d).astype(f32), (d * 2.0 / 886).astype(f32)
            pos = a[None, :].astype(np.float64) + np.arange(886)[:, None] * step[None, :].astype(np.float64)
            if not ((pos >= 0) & (pos <= 1)).all(1).any():
                continue
            crossing += 1
            pruned_hull += steps(lib, a, step, bs, planes, 886)[1] < 0
            pruned_box += steps(lib, a, step, bs, planes, 886, axes_only=True)[1] < 0
    assert crossing > 800
    assert pruned_hull > pruned_box + crossing // 10, (pruned_hull, pruned_box, crossing)


def test_empty_set_is_the_inverted_box_of_before(lib):
    """No active brick: every pair inverted.  The three axes answer as the box function did for the inverted box (a miss only where a
    step component is zero); the diagonals add a miss only where a ray does not move along one of them."""
    inv = bounds(lib, 2)
    assert (inv[:13] == f32(3.0e38)).all() and (inv[13:] == f32(-3.0e38)).all()
    box = np.array([3.0e38] * 3 + [-3.0e38] * 3, dtype=f32)
    bs = (16.0, 16.0, 16.0)
    rng = np.random.default_rng(3)
    k = np.zeros(2, dtype=np.int32)
    for i in range(2000):
        p = (rng.random(3) * 1.4 - 0.2).astype(f32)
        s = ((rng.random(3) - 0.5) * 0.004).astype(f32)
        if i % 4 == 1:
            s[rng.integers(3)] = 0
        if i % 4 == 2:
            s[1] = s[0]
        lib.hd_steps_box(ptr(p, C.c_float), ptr(s, C.c_float), ptr(box, C.c_float), 886, ptr(k, C.c_int))
        assert steps(lib, p, s, bs, inv, 886, axes_only=True) == (int(k[0]), int(k[1]))
        full = steps(lib, p, s, bs, inv, 886)
        if i % 4 in (1, 2):
            assert full == (0x7fffffff, -1)
        else:
            assert full == (0, 889) == (int(k[0]), int(k[1]))
    unb = bounds(lib, 1)
    assert steps(lib, (0.2, 0.3, 0.4), (0.001, 0.0, -0.001), bs, unb, 886) == (0, 889)
