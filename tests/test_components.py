"""CPU side of connected components (vr_mask_components): the restatement comp_ref.py, which the GPU tests compare the device with
element for element, pinned against scipy.ndimage.label (identical labels, not merely up to renaming), against grow_ref (a component is
the region grown from its first voxel), against scipy's binary_fill_holes for the hole-filling recipe, and against the laws of the
definition; the layout of the three new structs against the C compiler's, and the four exported symbols."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import comp_cases as cc
import comp_ref as cr
import grow_ref as gr
from volumerendering_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(5, 9, 70), (1, 12, 65), (7, 1, 64), (6, 6, 1), (4, 11, 130)]


def structure(connectivity):
    """scipy's structuring element of a connectivity."""
    s = np.zeros((3, 3, 3), bool)
    for dx, dy, dz in cr.offsets(connectivity):
        s[dz + 1, dy + 1, dx + 1] = True
    s[1, 1, 1] = True
    return s


@pytest.mark.parametrize("connectivity", cc.CONNECTIVITIES)
def test_labels_are_scipy_s(connectivity):
    ndi = pytest.importorskip("scipy.ndimage")
    seen = 0
    for k, shape in enumerate(SHAPES):
        for p in (0.1, 0.32, 0.5, 0.9):
            s = cc.random_set(shape, p, 100 * k + int(p * 100))
            want, n_want = ndi.label(s, structure(connectivity))
            got, n = cr.label(s, connectivity)
            assert n == n_want and np.array_equal(got, want), (shape, p, connectivity)
            seen = max(seen, n)
    for s in (cc.serpentine(), cc.comb(axis="row"), cc.comb(axis="slice"), cc.checkerboard(), cc.shells(), cc.corner_pair()):
        want, n_want = ndi.label(s, structure(connectivity))
        got, n = cr.label(s, connectivity)
        assert n == n_want and np.array_equal(got, want)
    assert seen > 50


def test_hand_made_shapes():
    assert cr.label(cc.serpentine(), cr.FACES)[1] == 1
    assert cr.label(cc.serpentine(), cr.PLANE_FACES)[1] == 5  # (three serpentine slices, and the two between them hold one voxel each)
    for axis in ("row", "slice"):
        a = cc.comb(axis=axis)
        assert cr.label(a, cr.FACES)[1] == (2 if axis == "row" else 1)
        cut = a.copy()
        if axis == "row":
            cut[:, -1, :] = False
        else:
            cut[-1] = False
        assert cr.label(cut, cr.FACES)[1] > 30
    b = cc.checkerboard()
    assert cr.label(b, cr.FACES)[1] == int(b.sum()) and cr.label(b, cr.ALL)[1] == 1
    s = cc.shells()
    assert cr.label(s, cr.ALL)[1] == 3 and cr.label(~s, cr.FACES)[1] == 4  # (three shells; the outside, two gaps and the centre)
    assert cr.label(cc.corner_pair(), cr.FACES)[1] == 2 and cr.label(cc.corner_pair(), cr.ALL)[1] == 1
    assert cr.label(cc.corner_pair(), cr.PLANE_ALL)[1] == 2


@pytest.mark.parametrize("connectivity", [cr.FACES, cr.ALL])
def test_a_component_is_the_region_grown_from_its_first(connectivity):
    shape = (5, 8, 66)
    s = cc.random_set(shape, 0.3 if connectivity == cr.FACES else 0.08, 5)
    lab, n = cr.label(s, connectivity)
    tab = cr.table(lab, n, (0, 0, 0))
    assert n > 20
    for i in range(0, n, max(1, n // 25)):
        assert np.array_equal(gr.region(s, [tab[i][3]], connectivity), lab == i + 1), i


def test_hole_filling_recipe():
    """Components of the complement that touch no face of the box, ORed in: binary_fill_holes in 3-D, and per slice with the PLANE
    connectivity and the four in-plane faces."""
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(9)
    shape = (9, 14, 67)
    a = ndi.binary_dilation(rng.random(shape) < 0.08, iterations=1)
    v = np.zeros(shape + (4,), np.float32)
    v[..., 0] = a
    got = cr.components(v, v, 0, 1, cr.FACES, *cc.whole(shape), reject_faces=63, dst_contour=0, combine=cr.OR)
    want = ndi.binary_fill_holes(a)
    assert np.array_equal(cr.member(got["out"][..., 0]), want) and want.sum() > a.sum()
    got = cr.components(v, v, 0, 1, cr.PLANE_FACES, *cc.whole(shape), reject_faces=15, dst_contour=0, combine=cr.OR)
    want = np.stack([ndi.binary_fill_holes(a[z]) for z in range(shape[0])])
    assert np.array_equal(cr.member(got["out"][..., 0]), want)


def test_laws_of_the_definition():
    shape = (6, 10, 70)
    box = ((3, 1, 1), (69, 9, 6))
    crop = (slice(1, 6), slice(1, 9), slice(3, 69))
    for seed, p in ((1, 0.2), (2, 0.33), (3, 0.6)):
        v = cc.volume(cc.random_set(shape, p, seed), 2, seed + 10)
        for connectivity in cc.CONNECTIVITIES:
            for background in (0, 1):
                got = cr.components(v, None, 2, background, connectivity, *box)
                tab, res = got["table"], got["result"]
                s = cr.member(v[..., 2])[crop] ^ bool(background)
                assert sum(t[0] for t in tab) == res[2] == int(s.sum()) and res[0] == len(tab)
                firsts = [(t[3][2] * shape[1] + t[3][1]) * shape[2] + t[3][0] for t in tab]
                assert firsts == sorted(firsts) and len(set(firsts)) == len(firsts)  # labels rise with `first`
                for i, t in enumerate(tab):
                    assert got["labels"][t[3][2], t[3][1], t[3][0]] == i + 1 and all(l <= f < h for l, f, h in zip(t[1], t[3], t[2]))
                assert not got["labels"][~np.pad(s, [(1, 0), (1, 1), (3, 1)])].any()
                nodes, pairs = got["counters"][1:]
                assert res[0] <= nodes <= res[2] and pairs >= nodes - res[0]  # (a spanning forest needs that many unions)
        # 26-components are unions of 6-components
        six = cr.components(v, None, 2, 0, cr.FACES, *box)["labels"]
        all26 = cr.components(v, None, 2, 0, cr.ALL, *box)["labels"]
        pairs = np.unique(np.stack([six[six > 0], all26[six > 0]]), axis=1)
        assert len(np.unique(pairs[0])) == pairs.shape[1]
        # selection is idempotent: the components of R under the same filters are R
        for filt in (dict(min_voxels=3), dict(keep_largest=2), dict(reject_faces=0b010101), dict(min_voxels=2, max_voxels=9, keep_largest=5)):
            first = cr.components(v, None, 2, 0, cr.FACES, *box, dst_contour=1, **filt)
            again = cr.components(first["out"], None, 1, 0, cr.FACES, *box, **filt)
            assert np.array_equal(again["r"], first["r"]) and again["result"][1] == again["result"][0] == first["result"][1]
    assert cr.select([(5, 0, 0, 0, 0), (7, 0, 0, 0, 0), (5, 0, 0, 0, 0), (7, 0, 0, 0, 0), (1, 0, 0, 0, 0)], keep_largest=3) == [0, 1, 3]
    assert cr.select([(5, 0, 0, 0, 0)], min_voxels=7, max_voxels=3) == []


def test_sweep_cases_cover_what_they_must():
    cases = cc.sweep(40)
    assert len(cases) == 40
    assert {c["connectivity"] for c in cases} == set(cc.CONNECTIVITIES) and {c["background"] for c in cases} == {0, 1}
    assert {c["shape"][2] for c in cases} == set(cc.NX) and {c["density"] for c in cases} >= {0.05, 0.3, 0.32, 0.35, 0.95}
    assert 1 in {c["shape"][1] for c in cases} and 1 in {c["shape"][0] for c in cases}
    written = [c for c in cases if c["dst_contour"] is not None]
    assert {c["combine"] for c in written} == {0, 1, 2, 3} and any(c["fresh"] for c in written)
    assert any(c["dst_slot"] == c["src_slot"] and c["dst_contour"] == c["src_contour"] for c in written)
    assert any(c["label_channel"] is not None and c["dst_contour"] is None for c in cases)
    assert any(c["label_channel"] is not None and c["dst_contour"] is not None for c in cases)
    assert any(c["dst_slot"] is None for c in cases) and any(c["box_hi"] != c["shape"][::-1] for c in cases)
    assert any(c["min_voxels"] > c["max_voxels"] for c in cases)
    ties = 0
    for c in cases[:12]:
        src, before = cc.case_volumes(c)
        got = cc.reference(c, src, before)
        assert got["result"][1] == len(got["selected"])
        if c["keep_largest"] and got["selected"]:
            sizes = sorted((t[0] for t in got["table"]), reverse=True)
            k = len(got["selected"])
            ties += k < len(sizes) and sizes[k - 1] == sizes[k]
    assert ties > 0  # (a tie at the K-th place is decided by the label)


def test_struct_layouts_match_the_header(tmp_path):
    fields = {"vr_component": ["voxels", "lo", "hi", "first", "faces"],
              "vr_components_desc": ["src_slot", "src_contour", "background", "connectivity", "box_lo", "box_hi", "min_voxels", "max_voxels",
                                     "reject_faces", "keep_largest", "dst_slot", "dst_contour", "combine", "label_slot", "label_channel",
                                     "max_components", "components"],
              "vr_components_result": ["n_components", "n_selected", "voxels", "selected_voxels", "largest", "lo", "hi"]}
    prints = "".join(f'printf("%zu ", sizeof({s}));' + "".join(f'printf("%zu ", offsetof({s}, {f}));' for f in fs) for s, fs in fields.items())
    consts = "VR_COMP_FACES, VR_COMP_ALL, VR_COMP_PLANE_FACES, VR_COMP_PLANE_ALL, VR_COMP_MAX_KEEP, (int)VR_COMP_MAX_LABEL"
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vr.h"\nint main(){' + prints +
                   'printf("%d %d %d %d %d %d", ' + consts + ');return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = []
    for s, fs in zip((capi.Component, capi.ComponentsDesc, capi.ComponentsResult), fields.values()):
        want += [C.sizeof(s)] + [getattr(s, f).offset for f in fs]
    assert out == want + [capi.COMP_FACES, capi.COMP_ALL, capi.COMP_PLANE_FACES, capi.COMP_PLANE_ALL, capi.COMP_MAX_KEEP, capi.COMP_MAX_LABEL]
    assert (cr.FACES, cr.ALL, cr.PLANE_FACES, cr.PLANE_ALL, cr.MAX_KEEP, cr.MAX_LABEL) == \
        (capi.COMP_FACES, capi.COMP_ALL, capi.COMP_PLANE_FACES, capi.COMP_PLANE_ALL, capi.COMP_MAX_KEEP, capi.COMP_MAX_LABEL)
    assert (cr.REPLACE, cr.OR, cr.AND, cr.ANDNOT) == (capi.MORPH_REPLACE, capi.MORPH_OR, capi.MORPH_AND, capi.MORPH_ANDNOT)
    assert C.sizeof(capi.Component) == 48  # (the device table is an array of it)


def test_library_exports_the_components_calls():
    lib = capi.load()
    for name in ("vr_components_whole", "vr_mask_components", "vr_components_counters", "vr_components_timing"):
        assert name in capi.ABI_SYMBOLS and hasattr(lib, name), name
    d = capi.ComponentsDesc().copy(box_lo=(1, 2, 3), box_hi=(4, 5, 6), connectivity=26, min_voxels=7, max_voxels=(1 << 64) - 1, dst_slot=-1)
    assert (tuple(d.box_lo), tuple(d.box_hi), d.connectivity, d.min_voxels, d.max_voxels, d.dst_slot) == \
        ((1, 2, 3), (4, 5, 6), 26, 7, (1 << 64) - 1, -1)
