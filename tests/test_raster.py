"""CPU side of polygon rasterisation (vr_mask_polygons): the restatement raster_ref.py, which the GPU tests compare the device with bit
for bit, pinned against an independent per-voxel crossing count in exact rationals, against closed forms, and (where matplotlib is
present) against matplotlib.path; the layout of the three new structs against the C compiler's, and the four exported symbols."""
import ctypes as C
import os
import subprocess
from fractions import Fraction as F

import numpy as np
import pytest

import raster_cases as rc
import raster_ref as rr
from volumerendering_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NX, NY = 14, 12


def covered_exact(points, origin, spacing, nx, ny):
    """The definition of include/vr.h, voxel by voxel: the number of edges with ay <= yc < by whose crossing lies strictly right of the
    centre, the crossing an exact rational."""
    p = [(int(x), int(y)) for x, y in np.asarray(points).reshape(-1, 2)]
    out = np.zeros((ny, nx), bool)
    for j in range(ny):
        yc = origin[1] + j * spacing[1]
        for i in range(nx):
            xc = origin[0] + i * spacing[0]
            n = 0
            for e in range(len(p)):
                (ax, ay), (bx, by) = p[e], p[(e + 1) % len(p)]
                if ay == by:
                    continue
                if ay > by:
                    ax, ay, bx, by = bx, by, ax, ay
                if ay <= yc < by and xc < ax + F((yc - ay) * (bx - ax), by - ay):
                    n += 1
            out[j, i] = n & 1
    return out


@pytest.mark.parametrize("grid", rc.GRIDS, ids=[f"{s[0]}x{s[1]}" + ("neg" if o[0] < 0 else "") for s, o in rc.GRIDS])
def test_restatement_equals_the_exact_crossing_count_on_the_tie_shapes(grid):
    spacing, origin = grid
    total = 0
    for name, shape in rc.tie_shapes():
        pts = rc.place(shape, origin, spacing)
        got = rr.polygon_rows(pts, origin, spacing, NX, NY)
        want = covered_exact(pts, origin, spacing, NX, NY)
        assert np.array_equal(got, want), (name, np.argwhere(got != want)[:4])
        if name in ("one_point", "two_points", "zero_area") or (name.startswith("between") and min(spacing) >= 4):
            assert not got.any(), name  # (on the unit grid the quarters of "between_*" round onto centres)
        total += int(got.sum())
    assert total > 200


def test_restatement_equals_the_exact_crossing_count_on_random_polygons():
    rng = np.random.default_rng(5)
    seen = 0
    for i in range(60):
        spacing, origin = rc.GRIDS[i % len(rc.GRIDS)]
        if i % 7 == 0:
            spacing, origin = (1 << 20, 1 << 20), (-(1 << 29), (1 << 29) - 11 * (1 << 20))  # (the range's corners)
        pts = rc.place(rc.random_polygon(rng, NX, NY, int(rng.integers(1, 25))), origin, spacing)
        pts = np.clip(pts, -rr.MAX_COORD, rr.MAX_COORD)
        got = rr.polygon_rows(pts, origin, spacing, NX, NY)
        assert np.array_equal(got, covered_exact(pts, origin, spacing, NX, NY)), i
        seen += int(got.any())
    assert seen > 30


def test_rows_are_the_prefix_toggles_of_edge_k():
    """polygon_rows, vectorised, against the same formulation edge by edge in Python integers (no int64 anywhere)."""
    rng = np.random.default_rng(6)
    for i in range(20):
        spacing, origin = rc.GRIDS[i % len(rc.GRIDS)]
        pts = rc.place(rc.random_polygon(rng, NX, NY, int(rng.integers(3, 40))), origin, spacing)
        p = [(int(x), int(y)) for x, y in pts]
        want = np.zeros((NY, NX), bool)
        for j in range(NY):
            for e in range(len(p)):
                k = rr.edge_k(*p[e], *p[(e + 1) % len(p)], origin[1] + j * spacing[1], origin[0], spacing[0], NX)
                if k is not None:
                    want[j, :k] ^= True
        assert np.array_equal(rr.polygon_rows(pts, origin, spacing, NX, NY), want), i


def ceil_div(a, b):
    return -((-a) // b)


@pytest.mark.parametrize("grid", rc.GRIDS[:3], ids=["unit", "ct", "aniso"])
def test_rectangle_covers_the_ceil_counted_centres(grid):
    """An axis-aligned rectangle [x0, x1) x [y0, y1) of the unit covers the centres with x0 <= xc < x1 and y0 <= yc < y1."""
    (sx, sy), (ox, oy) = grid
    rng = np.random.default_rng(7)
    for _ in range(30):
        x0, x1 = sorted(int(v) for v in rng.integers(ox - 2 * sx, ox + (NX + 2) * sx, 2))
        y0, y1 = sorted(int(v) for v in rng.integers(oy - 2 * sy, oy + (NY + 2) * sy, 2))
        if rng.random() < 0.5:  # (edges exactly on centres)
            (x0, x1), (y0, y1) = sorted((ox + 3 * sx, x1)), sorted((y0, oy + 9 * sy))
        got = rr.polygon_rows(rc.rect(x0, y0, x1, y1), (ox, oy), (sx, sy), NX, NY)
        i0, i1 = (min(max(ceil_div(v - ox, sx), 0), NX) for v in (x0, x1))
        j0, j1 = (min(max(ceil_div(v - oy, sy), 0), NY) for v in (y0, y1))
        want = np.zeros((NY, NX), bool)
        want[j0:j1, i0:i1] = True
        assert np.array_equal(got, want), (x0, y0, x1, y1)


def test_polygons_that_share_an_edge_partition_the_voxels():
    for spacing, origin in rc.GRIDS:
        # a slanted shared edge through voxel centres, and a vertical one on a column of centres
        for a, b, whole in [([(1, 1), (5, 1), (9, 9), (1, 9)], [(5, 1), (12, 1), (12, 9), (9, 9)], rc.rect(1, 1, 12, 9)),
                            (rc.rect(1, 1, 6, 9), rc.rect(6, 1, 12, 9), rc.rect(1, 1, 12, 9))]:
            ra, rb, rw = (rr.polygon_rows(rc.place(p, origin, spacing), origin, spacing, NX, NY) for p in (a, b, whole))
            assert not (ra & rb).any() and np.array_equal(ra | rb, rw) and ra.any() and rb.any()


def test_ring_is_a_hole_under_even_odd_and_solid_under_union():
    shape, origin, spacing = (3, NY, NX), (-500, 300), (500, 700)
    outer, inner = rc.place(rc.rect(1, 1, 12, 10), origin, spacing), rc.place(rc.ngon(9, 6, 5, 3, 2.5), origin, spacing)
    points, polygons = rc.flatten([(outer, 1, 2), (inner, 1, 2)])
    ro = rr.polygon_rows(outer, origin, spacing, NX, NY)
    ri = rr.polygon_rows(inner, origin, spacing, NX, NY)
    assert ri.any() and not (ri & ~ro).any()
    whole = ((0, 0, 0), (NX, NY, 3))
    for rule, want in ((rr.EVEN_ODD, ro & ~ri), (rr.UNION, ro)):
        out, result, r = rr.raster(shape, None, points, polygons, origin, spacing, 0b0100, rule, rr.REPLACE, *whole)
        assert np.array_equal(r[2, 1], want) and not r[2, 0].any() and not r[[0, 1, 3]].any()
        assert result[2][0] == int(want.sum()) and result[2][1] == (1, 1, 1) and result[2][2] == (12, 10, 2)
        assert np.array_equal(out[1, :, :, 2] == 1.0, want) and not out[..., [0, 1, 3]].any()


def test_combines_slices_and_the_box():
    """The four ways of storing on arbitrary bits, a polygon on a slice outside the box, the box cutting rows and columns."""
    import morph_cases as mc
    import vrtest as vt
    shape, origin, spacing = (4, NY, NX), (0, 0), (1, 1)
    before = mc.arbitrary_bits(shape, seed=3)
    points, polygons = rc.flatten([(rc.place(rc.rect(2, 2, 11, 9), origin, spacing), 1, 0), (rc.place(rc.rect(0, 0, 14, 12), origin, spacing), 3, 0),
                                   (rc.place(rc.rect(4, 1, 8, 11), origin, spacing), 2, 3)])
    lo, hi = (3, 1, 0), (10, 8, 3)
    for combine in (rr.REPLACE, rr.OR, rr.AND, rr.ANDNOT):
        out, result, r = rr.raster(shape, before, points, polygons, origin, spacing, 0b1001, rr.EVEN_ODD, combine, lo, hi)
        assert result[0] == (7 * 6, (3, 2, 1), (10, 8, 2)) and result[3] == (4 * 7, (4, 1, 2), (8, 8, 3)) and result[1] == result[2] == (0, (0, 0, 0), (0, 0, 0))
        assert np.array_equal(vt.bits(out[..., [1, 2]]), vt.bits(before[..., [1, 2]]))
        inbox = np.zeros(shape, bool)
        inbox[0:3, 1:8, 3:10] = True
        for k in (0, 3):
            b, a = vt.bits(before[..., k]), vt.bits(out[..., k])
            assert np.array_equal(a[~inbox], b[~inbox])
            want = {rr.REPLACE: np.where(r[k], rr.ONE, 0), rr.OR: np.where(r[k], rr.ONE, b), rr.AND: np.where(r[k], b, 0),
                    rr.ANDNOT: np.where(r[k], 0, b)}[combine]
            assert np.array_equal(a[inbox], want[inbox].astype(np.uint32))


def test_against_matplotlib_path():
    """Polygons whose edges keep every voxel centre at more than 1e-6 voxel: there the rule for ties cannot matter."""
    mpath = pytest.importorskip("matplotlib.path")
    rng = np.random.default_rng(8)
    nx, ny = 40, 32
    centres = np.stack(np.meshgrid(np.arange(nx, dtype=np.float64), np.arange(ny, dtype=np.float64)), -1).reshape(-1, 2)
    done = 0
    for i in range(200):
        spacing, origin = (977, 1013), (-33000, 12000)
        poly = rc.random_polygon(rng, nx, ny, int(rng.integers(3, 12)))
        pts = rc.place(poly, origin, spacing)
        v = (pts - np.asarray(origin)) / np.asarray(spacing, np.float64)  # voxel coordinates of the integer points
        a, b = v, np.roll(v, -1, axis=0)
        ab = b - a
        t = np.clip(((centres[:, None, :] - a[None]) * ab[None]).sum(-1) / np.maximum((ab * ab).sum(-1), 1e-30)[None], 0.0, 1.0)
        dist = np.linalg.norm(centres[:, None, :] - (a[None] + t[..., None] * ab[None]), axis=-1).min()
        if dist <= 1e-6:
            continue
        got = rr.polygon_rows(pts, origin, spacing, nx, ny)
        # (contains_points fills by the non-zero winding number: it agrees with even-odd on simple polygons only)
        if len(pts) > 3 and not _simple(v):
            continue
        want = mpath.Path(v).contains_points(centres).reshape(ny, nx)
        assert np.array_equal(got, want), i
        done += int(got.any())
    assert done > 20


def _simple(v):
    """No two non-adjacent edges of the closed polygon v (n, 2) cross or touch."""
    n = len(v)

    def orient(p, q, r):
        return np.sign((q[0] - p[0]) * (r[1] - p[1]) - (q[1] - p[1]) * (r[0] - p[0]))

    for i in range(n):
        for j in range(i + 1, n):
            if j == i or (j + 1) % n == i or (i + 1) % n == j:
                continue
            a, b, c, d = v[i], v[(i + 1) % n], v[j], v[(j + 1) % n]
            if orient(a, b, c) * orient(a, b, d) <= 0 and orient(c, d, a) * orient(c, d, b) <= 0:
                return False
    return True


def test_struct_layouts_match_the_header(tmp_path):
    fields = {"vr_polygon": ["first", "count", "slice", "contour"],
              "vr_polygons_desc": ["grid_slot", "dst_slot", "contours", "rule", "combine", "box_lo", "box_hi", "origin", "spacing", "n_points",
                                   "n_polygons", "points", "polygons"],
              "vr_polygons_result": ["voxels", "lo", "hi"]}
    prints = "".join(f'printf("%zu ", sizeof({s}));' + "".join(f'printf("%zu ", offsetof({s}, {f}));' for f in fs) for s, fs in fields.items())
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vr.h"\nint main(){' + prints + 'printf("%d %d", VR_POLY_EVEN_ODD, VR_POLY_UNION);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = []
    for s, fs in zip((capi.Polygon, capi.PolygonsDesc, capi.PolygonsResult), fields.values()):
        want += [C.sizeof(s)] + [getattr(s, f).offset for f in fs]
    assert out == want + [capi.POLY_EVEN_ODD, capi.POLY_UNION]
    assert (rr.EVEN_ODD, rr.UNION, rr.REPLACE, rr.OR, rr.AND, rr.ANDNOT) == (capi.POLY_EVEN_ODD, capi.POLY_UNION, capi.MORPH_REPLACE, capi.MORPH_OR,
                                                                               capi.MORPH_AND, capi.MORPH_ANDNOT)
    assert (rr.MAX_COORD, rr.MAX_SPACING) == (capi.POLY_MAX_COORD, capi.POLY_MAX_SPACING)


def test_library_exports_the_polygon_calls():
    lib = capi.load()
    for name in ("vr_polygons_whole", "vr_mask_polygons", "vr_polygons_counters", "vr_polygons_timing"):
        assert name in capi.ABI_SYMBOLS and hasattr(lib, name), name
    from volumerendering_amd import host
    hl = host.load()
    for name in ("vrh_app_raster_polygons", "vrh_app_contours_to_mask"):
        assert hasattr(hl, name), name
    d = capi.PolygonsDesc().copy(box_lo=(1, 2, 3), box_hi=(4, 5, 6), origin=(-7, 8), spacing=(9, 10), contours=5)
    assert (tuple(d.box_lo), tuple(d.box_hi), tuple(d.origin), tuple(d.spacing), d.contours) == ((1, 2, 3), (4, 5, 6), (-7, 8), (9, 10), 5)
    pts, polys = capi.polygon_arrays([(1, 2), (3, 4), (5, 6)], [(0, 3, 1, 2)])
    assert pts.dtype == np.int32 and pts.shape == (3, 2) and (polys[0].first, polys[0].count, polys[0].slice, polys[0].contour) == (0, 3, 1, 2)


def test_sweep_cases_are_legal_and_varied():
    cases = rc.sweep(40)
    assert len(cases) == 40
    assert {c["rule"] for c in cases} == {0, 1} and {c["combine"] for c in cases} == {0, 1, 2, 3}
    assert any(c["fresh"] for c in cases) and any(len(c["polygons"]) == 0 for c in cases) and max(len(c["polygons"]) for c in cases) > 40
    for c in cases:
        assert np.abs(c["points"]).max(initial=0) <= rr.MAX_COORD and all(1 <= s <= rr.MAX_SPACING for s in c["spacing"])
        assert all((c["contours"] >> k) & 1 for _, _, _, k in c["polygons"])
        assert all(1 <= n <= 90 for _, n, _, _ in c["polygons"])
