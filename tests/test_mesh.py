"""CPU side of surface extraction (vr_volume_mesh): the restatement mesh_ref.py, which the GPU tests compare the device with bit for
bit, pinned to facts that do not depend on it -- the counts, Euler characteristics and volumes of known surfaces, closedness, unique
directed edges, every vertex on its lattice edge between an inside and an outside point -- the layout of the two new structs against
the C compiler's, and the four exported symbols."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mesh_cases as mc
import mesh_ref as mr
from volumerendering_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name, field, level, cap, vertices, triangles, Euler characteristic, volume (None: not pinned), the volume is exact
KNOWN = [
    ("sphere", mc.sphere, 0.0, 0, 1466, 2928, 2, 513.17, False),
    ("torus", mc.torus, 0.0, 0, 1384, 2768, 0, None, False),
    ("one_voxel", mc.one_voxel, 0.5, 0, 14, 24, 2, 0.5, True),
    ("box_of_ones", mc.box_of_ones, 0.5, 1, 330, 656, 2, 24.0, True),
    ("random_mask", mc.random_mask, 0.5, 1, None, None, None, None, False),
]


def whole(v):
    return (0, 0, 0), v.shape[::-1]


def check_properties(v, level, cap, box_lo, box_hi, got, closed):
    """What the definition promises of any output."""
    verts, tris = got["vertices"], got["triangles"]
    n_v, n_t = got["result"][:2]
    assert verts.shape == (n_v, 3) and tris.shape == (n_t, 3) and verts.dtype == np.float32 and tris.dtype == np.uint32
    assert mr.edges_unique(tris)
    if closed:
        assert mr.is_closed(tris)
    if n_t:
        assert tris.max() < n_v and len(np.unique(tris)) == n_v  # every vertex is used
    lo, hi = np.array(box_lo), np.array(box_hi)

    def inside(p):
        return bool((lo <= p).all() and (p < hi).all() and v[p[2], p[1], p[0]] >= np.float32(level))

    keys = []
    for (p, m), pos in zip(got["edges"], verts.astype(np.float64)):
        p = np.array(p)
        d = np.array((m & 1, (m >> 1) & 1, m >> 2))
        assert 1 <= m <= 7 and inside(p) != inside(p + d)
        assert (p - cap >= lo - 2 * cap).all() and (p + d <= hi - 1 + cap).all()  # both ends are lattice points
        off = pos - p
        t = off[d == 1]
        ulp = float(np.spacing(np.float32(np.abs(pos).max())))  # (float)p + t is rounded once per axis
        assert (off[d == 0] == 0).all() and (np.abs(t - t[0]) <= ulp).all() and (0.0 <= t).all() and (t <= 1.0).all()  # on the edge
        l = p - (lo - cap)
        ln = hi - lo + 2 * cap
        keys.append(((int(l[2]) * int(ln[1]) + int(l[1])) * int(ln[0]) + int(l[0]), m))
    assert keys == sorted(keys) and len(set(keys)) == len(keys)


@pytest.mark.parametrize("case", KNOWN, ids=lambda c: c[0])
def test_known_answers(case):
    name, field, level, cap, n_v, n_t, chi, volume, exact = case
    v = field()
    got = mr.extract(v, level, cap, *whole(v))
    clear = name in ("sphere", "torus", "one_voxel")  # the surface is clear of the box
    check_properties(v, level, cap, *whole(v), got, closed=cap == 1 or clear)
    if n_v is not None:
        assert got["result"][:2] == (n_v, n_t)
        assert mr.euler(n_v, got["triangles"]) == chi
    vol = mr.signed_volume(got["vertices"], got["triangles"])
    assert vol > 0
    if volume is not None:
        assert vol == volume if exact else abs(vol - volume) < 0.005, vol
    assert got["result"][2] == int((v >= np.float32(level)).sum())


def test_sphere_volume_approaches_the_analytic_one():
    """The chordal mesh of a convex body lies inside it: at radius 5 on a unit lattice the prototype's gap to 4/3 pi r^3 = 523.6 is
    10.4 (2 %).  The gap of a piecewise-linear surface of a smooth body falls with the square of the cell size: a sphere of twice the radius
    on the same lattice must be at least 3 times closer in relative terms (4 in the limit)."""
    rel = []
    for n, r in ((14, 5.0), (26, 10.0)):
        v = mc.sphere(n, r)
        got = mr.extract(v, 0.0, 0, *whole(v))
        exact = 4.0 / 3.0 * np.pi * r ** 3
        vol = mr.signed_volume(got["vertices"], got["triangles"])
        assert vol < exact
        rel.append((exact - vol) / exact)
    assert rel[0] < 0.03 and rel[1] * 3 < rel[0], rel


def test_orientation_table_is_geometric():
    """Seen from outside, triangles are counter-clockwise: the normal of every triangle of the sphere points away from the centre."""
    v = mc.sphere()
    got = mr.extract(v, 0.0, 0, *whole(v))
    p = got["vertices"].astype(np.float64)[got["triangles"].astype(np.int64)]
    n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    assert (np.einsum("ij,ij->i", n, p.mean(1) - 6.5) > 0).all()
    assert len(mr.SWAP) == 6 * 14 and 0 < sum(mr.SWAP.values()) < 84


def test_boxes_caps_and_thin_lattices():
    v = mc.sphere()
    # a box that cuts the sphere: open without the cap, closed with it; the cap adds the cut faces
    box = ((3, 0, 2), (10, 14, 9))
    a = mr.extract(v, 0.0, 0, *box)
    b = mr.extract(v, 0.0, 1, *box)
    check_properties(v, 0.0, 0, *box, a, closed=False)
    check_properties(v, 0.0, 1, *box, b, closed=True)
    assert not mr.is_closed(a["triangles"]) and b["result"][1] > a["result"][1] and a["result"][2] == b["result"][2]
    assert mr.signed_volume(b["vertices"], b["triangles"]) > 0
    # a box thinner than 2 on an axis has no cells without the cap, and is a closed sheet with it
    thin = ((0, 0, 7), (14, 14, 8))
    assert mr.extract(v, 0.0, 0, *thin)["result"][:2] == (0, 0) and mr.extract(v, 0.0, 0, *thin)["result"][2] > 0
    c = mr.extract(v, 0.0, 1, *thin)
    check_properties(v, 0.0, 1, *thin, c, closed=True)
    assert c["result"][1] > 0
    # an empty box, and a level nothing reaches
    assert mr.extract(v, 0.0, 1, (4, 4, 4), (4, 9, 9))["result"] == (0, 0, 0, 0, (0, 0, 0), (0, 0, 0))
    assert mr.extract(v, 99.0, 1, *whole(v))["result"] == (0, 0, 0, 0, (0, 0, 0), (0, 0, 0))


def test_special_values():
    """Equal is in, NaN is out; infinities and a level on voxel values give vertices on lattice points and zero-area triangles that stay."""
    v = np.zeros((4, 4, 4), np.float32)
    v[1:3, 1:3, 1:3] = [[[1, np.inf], [np.nan, 1]], [[0.5, -0.0], [2, -np.inf]]]
    for level in (0.5, 0.0, 1.0):
        got = mr.extract(v, level, 1, *whole(v))
        check_properties(v, level, 1, *whole(v), got, closed=True)
        assert np.isfinite(got["vertices"]).all()
    got = mr.extract(v, 0.0, 0, *whole(v))  # -0.0 >= 0.0: everything but the NaN and -inf is inside
    assert got["result"][2] == 62


def test_sweep_cases_are_legal_and_varied():
    cases = mc.sweep(40)
    assert len(cases) == 40 and {c["cap"] for c in cases} == {0, 1} and {c["channel"] for c in cases} == {0, 1, 2, 3}
    assert {c["plain"] for c in cases} == {False, True}
    for c in cases:
        assert max(c["v"].shape) <= 40 and all(0 <= a <= b <= n for a, b, n in zip(c["box_lo"], c["box_hi"], c["v"].shape[::-1]))
    assert sum(mr.extract(c["v"], c["level"], c["cap"], c["box_lo"], c["box_hi"])["result"][1] > 0 for c in cases[:12]) >= 6


def test_struct_layouts_match_the_header(tmp_path):
    fields = {"vr_mesh_desc": ["src_slot", "channel", "level", "cap", "box_lo", "box_hi", "max_vertices", "max_triangles", "vertices", "triangles"],
              "vr_mesh_result": ["n_vertices", "n_triangles", "inside", "cells", "lo", "hi"]}
    prints = "".join(f'printf("%zu ", sizeof({s}));' + "".join(f'printf("%zu ", offsetof({s}, {f}));' for f in fs) for s, fs in fields.items())
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vr.h"\nint main(){' + prints + 'return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = []
    for s, fs in zip((capi.MeshDesc, capi.MeshResult), fields.values()):
        want += [C.sizeof(s)] + [getattr(s, f).offset for f in fs]
    assert out == want


def test_library_exports_the_mesh_calls():
    lib = capi.load()
    for name in ("vr_mesh_whole", "vr_volume_mesh", "vr_mesh_counters", "vr_mesh_timing"):
        assert name in capi.ABI_SYMBOLS and hasattr(lib, name), name
    from volumerendering_amd import host
    hl = host.load()
    for name in ("vrh_app_extract_surface", "vrh_mesh_write_stl", "vrh_mesh_write_ply"):
        assert hasattr(hl, name), name
    d = capi.MeshDesc().copy(box_lo=(1, 2, 3), box_hi=(4, 5, 6), channel=2, level=0.25, cap=1)
    assert (tuple(d.box_lo), tuple(d.box_hi), d.channel, d.level, d.cap) == ((1, 2, 3), (4, 5, 6), 2, 0.25, 1)
