"""CPU side of contour tracing (vr_mask_outlines): the restatement outline_ref.py, which the GPU tests compare the device with element
for element, pinned against a sequential crack walker that follows successors from the smallest unvisited key, against raster_ref (the
outlines, rasterised even-odd, give the set back), against closed forms, and the properties of the definition; the layout of the two
new structs against the C compiler's, and the four exported symbols."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import outline_cases as oc
import outline_ref as orf
import raster_ref as rr
from volumerendering_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def one_slice(s):
    """A boolean (ny, nx) slice as the members (4, 1, ny, nx) of contour 0."""
    m = np.zeros((4, 1) + s.shape, bool)
    m[0, 0] = s
    return m


def whole(m):
    return (0, 0, 0), m.shape[:0:-1]


def same(got, points, polygons):
    return np.array_equal(got["points"], points) and got["polygons"] == polygons


def check_properties(m, contours, box_lo, box_hi, got, grid=((1, 1), (0, 0)), offset=(0, 0)):
    """What the definition promises of an output: area2 == 2 |S|, first point lowest-then-leftmost, alternating axis-parallel steps, an
    even count of at least 4, the order of the polygons, `first` running."""
    pts, polys = got["points"].astype(np.int64), got["polygons"]
    n_points, n_polygons, polygons_of, points_of, area2 = got["result"]
    assert n_points == len(pts) and n_polygons == len(polys)
    nx = m.shape[3]
    (sx, sy), (ox, oy) = grid
    crop = (slice(box_lo[2], box_hi[2]), slice(box_lo[1], box_hi[1]), slice(box_lo[0], box_hi[0]))
    keys, run = [], 0
    for first, count, z, k in polys:
        assert first == run and count >= 4 and count % 2 == 0 and (contours >> k) & 1 and box_lo[2] <= z < box_hi[2]
        run += count
        p = pts[first:first + count]
        step = np.roll(p, -1, axis=0) - p
        assert ((step != 0).sum(1) == 1).all()                          # consecutive points differ in exactly one coordinate ...
        along = (step[:, 1] != 0).astype(int)
        assert (along != np.roll(along, -1)).all()                       # ... alternating
        order = np.lexsort((p[:, 0], p[:, 1]))
        assert order[0] == 0                                             # the first point is the lowest, then the leftmost
        i, j = (p[0, 0] - ox + offset[0]) // sx, (p[0, 1] - oy + offset[1]) // sy
        assert step[0, 0] > 0 or step[0, 1] > 0
        keys.append((k, z, (j * (nx + 1) + i) * 4 + (0 if step[0, 0] else 1)))
    assert run == len(pts) and keys == sorted(keys) and len(set(keys)) == len(keys)
    for k in range(4):
        mine = [q for q in polys if q[3] == k]
        assert polygons_of[k] == len(mine) and points_of[k] == sum(q[1] for q in mine)
        want = 2 * int(m[k][crop].sum()) if (contours >> k) & 1 else 0
        assert area2[k] == want, (k, area2[k], want)
        shoelace = 0
        for first, count, _, _ in mine:
            p = pts[first:first + count]
            q = np.roll(p, -1, axis=0)
            shoelace += int((p[:, 0] * q[:, 1] - q[:, 0] * p[:, 1]).sum())
        assert shoelace == want * sx * sy


def rasterised(got, shape, grid, contours, box_lo, box_hi):
    """The polygons of an output, XORed per contour and slice by raster_ref.polygon_rows: boolean (4, nz, ny, nx)."""
    nz, ny, nx = shape
    r = np.zeros((4, nz, ny, nx), bool)
    for first, count, z, k in got["polygons"]:
        r[k, z] ^= rr.polygon_rows(got["points"][first:first + count], grid[1], grid[0], nx, ny)
    return r


@pytest.mark.parametrize("case", oc.slices_with_known_outlines(), ids=lambda c: c[0])
def test_known_outlines(case):
    name, s, n_split, n_join, p_split, p_join = case
    m = one_slice(s)
    for connect, n_poly, n_pts in ((orf.SPLIT, n_split, p_split), (orf.JOIN, n_join, p_join)):
        got = orf.trace(m, 1, connect, *whole(m))
        assert same(got, *oc.walk_volume(m, 1, connect, *whole(m))), (name, connect)
        check_properties(m, 1, *whole(m), got)
        if n_poly is not None:
            assert got["result"][1] == n_poly, (name, connect, got["result"])
        assert got["result"][0] == n_pts, (name, connect, got["result"])
    if name == "single_voxel":
        assert got["points"].tolist() == [[1, 1], [2, 1], [2, 2], [1, 2]] and got["polygons"] == [(0, 4, 0, 0)]
    if name == "one_voxel_hole":  # the outer boundary counter-clockwise, the hole clockwise
        assert got["points"].tolist() == [[0, 0], [5, 0], [5, 5], [0, 5], [2, 2], [2, 3], [3, 3], [3, 2]]
    if name == "diagonal":  # JOIN: one polygon of 8 points through the shared vertex twice
        assert got["points"].tolist() == [[1, 1], [2, 1], [2, 2], [3, 2], [3, 3], [2, 3], [2, 2], [1, 2]]


@pytest.mark.parametrize("nx", [1, 63, 64, 65, 128])
def test_word_edges_against_the_walker(nx):
    """Rows of 1, 63, 64, 65 and 128 voxels (64 already needs a second vertex word), full, random and checkerboard, boxes that cut."""
    rng = np.random.default_rng(nx)
    ny = 7
    full = np.ones((4, 2, ny, nx), bool)
    board = np.broadcast_to((np.add.outer(np.arange(ny), np.arange(nx)) & 1) == 0, (4, 2, ny, nx)).copy()
    rand = rng.random((4, 2, ny, nx)) < 0.5
    for m in (full, board, rand):
        boxes = [whole(m), ((0, 1, 0), (nx, ny - 1, 2)), ((nx // 2, 0, 1), (nx, ny, 2)), ((0, 0, 0), (max(nx - 1, 0), 3, 1)), ((nx - 1, 2, 0), (nx, 5, 2))]
        for box in boxes:
            for connect in (orf.SPLIT, orf.JOIN):
                got = orf.trace(m, 0b0101, connect, *box)
                assert same(got, *oc.walk_volume(m, 0b0101, connect, *box)), (nx, box, connect)
                check_properties(m, 0b0101, *box, got)
    assert orf.trace(full, 1, 0, *whole(full))["points"][:4].tolist() == [[0, 0], [nx, 0], [nx, ny], [0, ny]]


@pytest.mark.parametrize("g", range(4), ids=["unit", "ct_negative", "aniso_negative", "unit_negative"])
def test_raster_of_the_outlines_is_the_set(g):
    """XOR of raster_ref.polygon_rows over the polygons equals S for offsets 0, spacing - 1 and spacing / 2, under both rules, on boxes
    that cut the structures."""
    grid = oc.GRIDS[g]
    shape = (2, 23, 70)
    for seed, m in ((1, oc.blobs(shape, 11 + g)), (2, oc.random_members(shape, 0.5, 17 + g))):
        for box in (((0, 0, 0), (70, 23, 2)), ((5, 3, 1), (66, 20, 2))):
            inbox = np.zeros(shape, bool)
            inbox[box[0][2]:box[1][2], box[0][1]:box[1][1], box[0][0]:box[1][0]] = True
            for offset in oc.offsets(grid[0]):
                for connect in (orf.SPLIT, orf.JOIN):
                    got = orf.trace(m, 15, connect, *box, origin=grid[1], spacing=grid[0], offset=offset)
                    assert same(got, *oc.walk_volume(m, 15, connect, *box, grid[1], grid[0], offset))
                    assert np.array_equal(rasterised(got, shape, grid, 15, *box), m & inbox[None]), (g, seed, box, offset, connect)
                    check_properties(m, 15, *box, got, grid, offset)


def test_rounds_of_the_two_forms_and_long_loops():
    """The default form stops after the first round that changes nothing, the plain form runs ceil(log2(nodes)) rounds: same output.
    The seeds of the GPU test's long loops hold its condition."""
    for p, connect, seed in ((0.6, orf.SPLIT, 7), (0.5, orf.JOIN, 7)):
        m = oc.random_members((2, 140, 140), p, seed)
        a = orf.trace(m, 1, connect, *whole(m))
        b = orf.trace(m, 1, connect, *whole(m), plain=True)
        assert same(a, b["points"], b["polygons"]) and a["result"] == b["result"]
        assert a["longest"] >= 1024 and a["rounds"] < b["rounds"], (a["longest"], a["rounds"], b["rounds"])
        assert b["rounds"] == int(np.ceil(np.log2(a["result"][0])))
        check_properties(m, 1, *whole(m), a)


def test_empty_inputs_give_no_polygons():
    m = oc.random_members((2, 5, 9), 0.5, 3)
    assert orf.trace(m, 1, 0, (0, 0, 0), (9, 5, 0))["result"] == (0, 0, (0,) * 4, (0,) * 4, (0,) * 4)
    assert orf.trace(m, 1, 0, (4, 0, 0), (4, 5, 2))["polygons"] == []
    m[2] = False
    assert orf.trace(m, 0b0100, 1, *whole(m))["result"][0] == 0
    assert orf.member(np.array([np.nan, -0.0, 0.0, 1e-45, -1.0], np.float32)).tolist() == [True, False, False, True, True]
    v = oc.volume(m, seed=4)
    assert np.array_equal(orf.members(v), m) and np.isnan(v).any() and np.signbit(v[v == 0]).any()


def test_sweep_cases_are_legal_and_varied():
    cases = oc.sweep(40)
    assert len(cases) == 40 and {c["connect"] for c in cases} == {0, 1} and {c["plain"] for c in cases} == {False, True}
    assert len({c["contours"] for c in cases}) > 8
    for c in cases:
        assert all(0 <= o < s <= orf.MAX_SPACING for o, s in zip(c["offset"], c["spacing"]))
    for c in cases[:6]:
        got = orf.trace(c["m"], c["contours"], c["connect"], c["box_lo"], c["box_hi"], c["origin"], c["spacing"], c["offset"], c["plain"])
        assert same(got, *oc.walk_volume(c["m"], c["contours"], c["connect"], c["box_lo"], c["box_hi"], c["origin"], c["spacing"], c["offset"]))


def test_struct_layouts_match_the_header(tmp_path):
    fields = {"vr_outlines_desc": ["src_slot", "contours", "connect", "box_lo", "box_hi", "origin", "spacing", "offset", "max_points", "max_polygons",
                                   "points", "polygons"],
              "vr_outlines_result": ["n_points", "n_polygons", "polygons_of", "points_of", "area2"]}
    prints = "".join(f'printf("%zu ", sizeof({s}));' + "".join(f'printf("%zu ", offsetof({s}, {f}));' for f in fs) for s, fs in fields.items())
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vr.h"\nint main(){' + prints + 'printf("%d %d", VR_OUTLINE_SPLIT, VR_OUTLINE_JOIN);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = []
    for s, fs in zip((capi.OutlinesDesc, capi.OutlinesResult), fields.values()):
        want += [C.sizeof(s)] + [getattr(s, f).offset for f in fs]
    assert out == want + [capi.OUTLINE_SPLIT, capi.OUTLINE_JOIN]
    assert (orf.SPLIT, orf.JOIN, orf.MAX_COORD, orf.MAX_SPACING) == (capi.OUTLINE_SPLIT, capi.OUTLINE_JOIN, capi.POLY_MAX_COORD, capi.POLY_MAX_SPACING)


def test_library_exports_the_outline_calls():
    lib = capi.load()
    for name in ("vr_outlines_whole", "vr_mask_outlines", "vr_outlines_counters", "vr_outlines_timing"):
        assert name in capi.ABI_SYMBOLS and hasattr(lib, name), name
    from volumerendering_amd import host
    hl = host.load()
    for name in ("vrh_app_mask_outlines", "vrh_app_mask_to_contours"):
        assert hasattr(hl, name), name
    d = capi.OutlinesDesc().copy(box_lo=(1, 2, 3), box_hi=(4, 5, 6), origin=(-7, 8), spacing=(9, 10), offset=(4, 5), contours=5, connect=1)
    assert (tuple(d.box_lo), tuple(d.box_hi), tuple(d.origin), tuple(d.spacing), tuple(d.offset), d.contours, d.connect) == \
        ((1, 2, 3), (4, 5, 6), (-7, 8), (9, 10), (4, 5), 5, 1)
