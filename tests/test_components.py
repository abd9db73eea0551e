"""CPU side of connected components (vr_mask_components): the restatement comp_ref.py, which the GPU tests compare the device with
element for element, pinned against scipy.ndimage.label (identical labels, not merely up to renaming), against grow_ref (a component is
the region grown from its first voxel), against scipy's binary_fill_holes for the hole-filling recipe, and against the laws of the
definition; the layout of the three new structs against the C compiler's, and the four exported symbols.  For the scale tests
(tests/test_components_scale_gpu.py): their thresholds against the headers, what each of their cases must contain, and their
vectorised table and closed-form labels against the restatement."""
import ctypes as C
import os
import re
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


def test_table_arrays_is_table_on_the_sweep():
    """comp_ref.table_arrays, which the scale tests read, equals comp_ref.table on every case of the sweep, and comp_cases'
    reference_arrays equals comp_ref.components: result, counters, selection and the written slot bit for bit."""
    seen = 0
    for c in cc.sweep(40):
        src, before = cc.case_volumes(c)
        want = cc.reference(c, src, before)
        got = cc.reference_arrays(src, before, c["src_contour"], c["background"], c["connectivity"], c["box_lo"], c["box_hi"],
                                  c["min_voxels"], c["max_voxels"], c["reject_faces"], c["keep_largest"], c["dst_contour"], c["combine"],
                                  c["label_channel"])
        voxels, lo, hi, first, faces = got["table"]
        rows = [(int(voxels[i]), tuple(lo[i].tolist()), tuple(hi[i].tolist()), tuple(first[i].tolist()), int(faces[i])) for i in range(len(voxels))]
        assert rows == want["table"], c
        assert got["result"] == want["result"] and got["counters"] == want["counters"] and got["selected"].tolist() == want["selected"], c
        assert np.array_equal(got["labels"], want["labels"]) and np.array_equal(got["r"], want["r"])
        assert (got["out"] is None) == (want["out"] is None)
        if want["out"] is not None:
            assert np.array_equal(got["out"].view(np.uint32), want["out"].view(np.uint32)), c
        seen += len(rows)
    assert seen > 1000
    assert all(len(col) == 0 for col in cr.table_arrays(np.zeros((2, 3, 4), np.int64), 0, (0, 0, 0)))


def test_scale_thresholds_are_the_headers():
    """The sizes the scale cases are built around, read from the sources: a retune fails here instead of leaving the cases below it."""
    def text(name):
        with open(os.path.join(ROOT, "volumerendering_amd", "csrc", name)) as f:
            return f.read()

    scan, api_tools = text("vr_scan.h"), text("vr_api_tools.h")
    assert int(re.search(r"constexpr int kScanTile = (\d+);", scan).group(1)) == cc.SCAN_TILE
    spine = scan[scan.index("void scan_spine_kernel"):scan.index("void scan_apply_kernel")]
    assert int(re.search(r"for \(unsigned long long b0 = 0; b0 < nb; b0 \+= (\d+)u\)", spine).group(1)) == cc.SPINE_CHUNK
    assert "__shared__ unsigned long long s[%d];" % cc.SPINE_CHUNK in spine
    assert int(re.search(r"constexpr unsigned kToolBlocks = (\d+);", api_tools).group(1)) == cc.TOOL_BLOCKS
    m = re.search(r"unsigned lane_blocks\(unsigned long long n\) \{ return \(unsigned\)std::min<unsigned long long>\("
                  r"\(n \+ 255ull\) / 256ull, (\d+)ull \* kToolBlocks\); \}", api_tools)
    assert int(m.group(1)) * cc.TOOL_BLOCKS * 256 == cc.LANE_CAP == 524288
    m = re.search(r"unsigned tool_blocks\(unsigned long long n\) \{ return n < (\d+) \? 1u : \(n / (\d+) < kToolBlocks \? "
                  r"\(unsigned\)\(n / (\d+)\) : kToolBlocks\); \}", api_tools)
    assert {int(g) for g in m.groups()} == {4} and 4 * cc.TOOL_BLOCKS == cc.WORDS_PER_PASS == 2048
    comp = text("vr_comp.h") + text("vr_api_components.h")  # (its pack and its scans are launched by vr_api_tools.h's tool_pack, tool_scan)
    assert (comp + api_tools).count("dim3(256)") >= 14 and "dim3(lane_blocks(" in comp and "dim3(tool_blocks(bwords))" in comp
    assert "tool_pack(" in comp and comp.count("tool_scan(") == 2 and "dim3(tool_blocks(b.box_words))" in api_tools
    assert cc.SCAN_TILE * cc.SPINE_CHUNK == 262144


def column_runs(s, axis_rows):
    """[(first, last)] of the runs along x of one row of s."""
    row = np.concatenate(([False], s[axis_rows], [False]))
    edges = np.flatnonzero(row[1:] != row[:-1])
    return list(zip(edges[::2].tolist(), (edges[1::2] - 1).tolist()))


@pytest.mark.parametrize("name", list(cc.RODS))
def test_rods_hold_what_they_must(name):
    """The 65535-voxel rods of the scale tests: what each must contain, from the restatement alone."""
    a = cc.rod(name)
    shape = cc.RODS[name]
    assert a.shape == shape and max(shape) == cc.AXIS and sorted(shape)[1] <= 3 and shape[::-1][cc.rod_axis(name)] == cc.AXIS
    (lo, hi), (cut_lo, cut_hi) = cc.rod_boxes(name)
    k = cc.rod_axis(name)
    assert (lo, hi) == cc.whole(shape) and cut_lo[k] == 1 and cut_hi[k] == cc.AXIS - 1
    assert all(cut_lo[i] == lo[i] and cut_hi[i] == hi[i] for i in range(3) if i != k)
    lab, n = cr.label(a, cr.FACES)
    nodes, _ = cr.run_counts(a, cr.FACES)
    if name[0] == "x":
        rows = a.reshape(-1, cc.AXIS)
        runs = [column_runs(rows, r) for r in range(rows.shape[0])]
        every = [run for r in runs for run in r]
        assert [(0, cc.AXIS - 1)] in runs                                   # the whole row
        assert (cc.AXIS - 1, cc.AXIS - 1) in every and (0, 63) in every     # a one-voxel run at the far end; a run that ends a word
        assert (64, 64) in every and (name == "x" or any(f == 64 and l > 127 for f, l in every))  # runs that start one
        assert max(len(r) for r in runs) >= 32768 and nodes == len(every)
        assert n >= 1000
        # the full row joins what lies more than 1000 words apart: the two ends of the row beside it are one component with it, two without
        full = runs.index([(0, cc.AXIS - 1)])
        near, far = np.unravel_index((full + 1) * cc.AXIS + 0, shape), np.unravel_index((full + 1) * cc.AXIS + cc.AXIS - 1, shape)
        assert a[near] and a[far] and (cc.AXIS - 1) // 64 - 0 > 1000
        assert lab[near] == lab[far] == lab.reshape(-1, cc.AXIS)[full, 0]
        cut = a.copy()
        cut.reshape(-1, cc.AXIS)[full] = False
        without = cr.label(cut, cr.FACES)[0]
        assert without[near] != without[far]
        # ... and it does not swallow everything: many rows' runs stay apart from it
        assert np.count_nonzero(np.bincount(lab.ravel())[1:] == 1) >= 1000
        # the cut box: a partial first word from word 0, and hi[0] = 65534
        assert cut_lo[0] // 64 == 0 and cut_lo[0] % 64 == 1 and cut_hi[0] == 65534
    else:
        cols = np.moveaxis(a, 0 if name == "z" else 1, -1).reshape(-1, cc.AXIS)
        counts = sorted(len(column_runs(cols, r)) for r in range(cols.shape[0]) if cols[r].any())
        assert counts[0] == 1 and cols.all(axis=1).sum() == 1           # a full-length column: 65535 nodes of one component
        assert counts[-1] == 32768                                       # every other voxel
        assert 10000 < counts[1] < 30000                                 # a seeded one
        assert n > 10000 and int(np.bincount(lab.ravel())[1:].max()) == cc.AXIS and nodes == int(a.sum())
        if name == "z":
            assert cr.label(a, cr.PLANE_FACES)[1] >= cc.AXIS  # (no path crosses slices)
            assert cr.label(a, cr.PLANE_FACES)[1] == int(a.sum())


MIDDLE_COUNTS = {"checkerboard_faces": (1048576, 0, 1048576, 1), "checkerboard_all": (1048576, 6193536, 1, 1048576),
                 "columns": (1048576, 2080768, 64, 16384), "blobs": (553693, 341864, 225615, 305)}  # nodes, pairs, components, largest


@pytest.mark.parametrize("name", list(cc.MIDDLE))
def test_middle_scale_cases_exceed_the_lane_cap(name):
    """Every middle-scale mask puts more than LANE_CAP nodes through the kernels, the FACES checkerboard as many components and more
    than one spine chunk of them; the seeded blobs (density 0.25, FACES) are there for their wavefronts of many small and mid-sized
    components."""
    make, connectivity, keep = cc.MIDDLE[name]
    a = make()
    nodes, pairs = cr.run_counts(a, connectivity)
    lab, n = cr.label(a, connectivity)
    assert (nodes, pairs, n, int(np.bincount(lab.ravel())[1:].max())) == MIDDLE_COUNTS[name]
    assert a.size * 16 <= 45 << 20 and 1 <= keep <= cr.MAX_KEEP and nodes > cc.LANE_CAP
    if name == "checkerboard_faces":
        assert n > cc.LANE_CAP and n > cc.SCAN_TILE * cc.SPINE_CHUNK


def test_scan_edge_boxes_have_the_words_they_must():
    one = cc.SCAN_TILE * cc.SPINE_CHUNK
    assert cc.SCAN_SHAPE[2] <= 64 and cc.SCAN_SHAPE[0] * cc.SCAN_SHAPE[1] * cc.SCAN_SHAPE[2] * 16 <= 36 << 20
    assert cc.box_words(cc.SCAN_SHAPE, *cc.SCAN_BOXES["one_chunk"]) == one == 262144
    assert cc.box_words(cc.SCAN_SHAPE, *cc.SCAN_BOXES["one_more"]) == one + 1
    for lo, hi in cc.SCAN_BOXES.values():
        assert all(0 <= l < h <= n for l, h, n in zip(lo, hi, cc.SCAN_SHAPE[::-1]))
    assert cc.box_words((5, 9, 130), (63, 0, 0), (65, 9, 5)) == 2 * 9 * 5 and cc.box_words((5, 9, 130), (3, 2, 1), (3, 9, 5)) == 0
    a = cc.random_set(cc.SCAN_SHAPE, cc.SCAN_DENSITY, cc.SCAN_SEED)
    for lo, hi in cc.SCAN_BOXES.values():  # the second scan, over the nodes, goes beyond one chunk too
        nodes, _ = cr.run_counts(a[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]], cr.FACES)
        assert nodes > one + cc.SCAN_TILE


def test_isolated_labels_is_the_restatement():
    """The closed form the label-limit test compares with (comp_cases.isolated_labels), pinned to comp_ref.components on a checkerboard
    with a box; and the sizes of that test: 128 slices hold exactly 2^24 isolated voxels, 129 hold 131 072 more."""
    shape = (6, 8, 70)
    a = cc.checkerboard(shape)
    v = np.zeros(shape + (4,), np.float32)
    v[..., 0] = a
    box_lo, box_hi = (3, 1, 1), (69, 8, 5)
    crop = (slice(1, 5), slice(1, 8), slice(3, 69))
    got = cr.components(v, None, 0, 0, cr.FACES, box_lo, box_hi)
    want = cc.isolated_labels(a[crop])
    n = int(a[crop].sum())
    assert np.array_equal(got["labels"][crop], want) and got["result"][:5] == (n, n, n, n, 1) and got["counters"] == (a[crop].size, n, 0)
    z, y, x = np.nonzero(a[crop])
    first = [(int(i) + 3, int(j) + 1, int(k) + 1) for i, j, k in zip(x, y, z)]
    assert [t[3] for t in got["table"]] == first and all(t[0] == 1 and t[1] == t[3] and t[2] == tuple(q + 1 for q in t[3]) for t in got["table"])
    nz, ny, nx = cc.LIMIT_SHAPE
    assert ny * nx // 2 == 131072 and 128 * ny * nx // 2 == cr.MAX_LABEL and 129 * ny * nx // 2 == cr.MAX_LABEL + 131072 and nz == 130
    assert np.float32(cr.MAX_LABEL - 1) != np.float32(cr.MAX_LABEL) and np.float32(cr.MAX_LABEL + 1) == np.float32(cr.MAX_LABEL)


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
