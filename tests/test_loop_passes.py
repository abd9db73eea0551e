"""CPU side of the loop-pass cases (tests/loop_cases.py): the thresholds and the launch of every kernel read from the headers, a row of
the inventory for every grid-stride loop the headers have, every row's case at least two passes long with a partial last one and with
content in the words or units of the later passes, the fishbone's single loop, and the band-by-band mesh reference pinned to
mesh_ref.extract."""
import os
import re

import numpy as np
import pytest

import comp_ref as cr
import loop_cases as lc
import mesh_cases as mcs
import mesh_ref as mr
import outline_cases as oc
import outline_ref as orf
import raster_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the host file that launches a header's kernels
API = {"vr_bitrows.h": "vr_api_tools.h", "vr_morph.h": "vr_api_morph.h", "vr_dist.h": "vr_api_dist.h", "vr_raster.h": "vr_api_raster.h",
       "vr_outline.h": "vr_api_outline.h", "vr_mesh.h": "vr_api_mesh.h", "vr_hist.h": "vr_api_views.h", "vr_grow.h": "vr_api_segment.h",
       "vr_resample.h": "vr_api_resample.h", "vr_comp.h": "vr_api_components.h"}
TRACES = {}


def text(name):
    with open(os.path.join(ROOT, "volumerendering_amd", "csrc", name)) as f:
        return f.read()


def loops_of(header):
    """[(kernel, the loop's line, what the loop's step is made of)] for every grid-stride loop of a header, in order."""
    out, kernel, per = [], None, None
    for line in text(header).splitlines():
        m = re.search(r"__global__.* void (\w+)\(", line)
        if m:
            kernel, per = m.group(1), None
        m = re.search(r"(?:W|stride) = .*gridDim\.x \* (4|256)", line)
        if m:
            per = int(m.group(1))
        if re.search(lc.LOOP, line):
            out.append((kernel, line, per))
    return out


def trace(name):
    if name not in TRACES:
        m, shape, connect = {"fish": (lc.fishbone_members(), lc.FISH_SHAPE, orf.SPLIT),
                             "board_split": (lc.board_members(), lc.BOARD_SHAPE, orf.SPLIT),
                             "board_join": (lc.board_members(), lc.BOARD_SHAPE, orf.JOIN)}[name]
        TRACES[name] = (m, orf.trace(m, 1, connect, (0, 0, 0), shape[::-1]))
    return TRACES[name]


def test_thresholds_and_launches_are_the_headers():
    """kToolBlocks and the two rules as comp_cases states them (tests/test_components.py reads the same lines), the rows of an item, and
    for every row of the inventory the launch of its kernel under the rule the row names."""
    api_tools = text("vr_api_tools.h")
    assert int(re.search(r"constexpr unsigned kToolBlocks = (\d+);", api_tools).group(1)) == lc.TOOL_BLOCKS
    m = re.search(r"unsigned lane_blocks\(unsigned long long n\) \{ return \(unsigned\)std::min<unsigned long long>\("
                  r"\(n \+ 255ull\) / 256ull, (\d+)ull \* kToolBlocks\); \}", api_tools)
    assert int(m.group(1)) * lc.TOOL_BLOCKS * 256 == lc.LANE_CAP
    m = re.search(r"unsigned tool_blocks\(unsigned long long n\) \{ return n < (\d+) \? 1u : \(n / (\d+) < kToolBlocks \? "
                  r"\(unsigned\)\(n / (\d+)\) : kToolBlocks\); \}", api_tools)
    assert {int(g) for g in m.groups()} == {4} and 4 * lc.TOOL_BLOCKS == lc.WORDS_PER_PASS
    for n in (0, 3, 4, 7, 2047, 2048, 2049, 4097, 1 << 20):
        assert lc.tool_blocks(n) == (1 if n < 4 else min(n // 4, 512)) and lc.lane_blocks(n) == min((n + 255) // 256, 2048)
    assert lc.passes("tool", 2048) == (1, 2048, 2048) and lc.passes("tool", 4097) == (3, 1, 2048)
    assert lc.passes("lane", lc.LANE_CAP) == (1, lc.LANE_CAP, lc.LANE_CAP) and lc.passes("lane", lc.LANE_CAP + 1)[:2] == (2, 1)
    assert int(re.search(r"constexpr int kRasterRowsPerItem = (\d+);", text("vr_api_raster.h")).group(1)) == lc.ROWS_PER_ITEM
    for row in lc.ROWS:
        api = text(API[row["header"]])
        rule = row["rule"] + "_blocks("
        if row["kernel"] == "resample_kernel":  # (launched through the per-arithmetic launcher: the grid is computed here)
            assert "const unsigned blocks = tool_blocks(R.units);" in api
            continue
        at = api.index("hipLaunchKernelGGL(" + row["kernel"])
        grid = re.match(r"[\w<>]+, dim3\(([^;]*?)\), dim3\(256\)", api[at + len("hipLaunchKernelGGL("):]).group(1)
        if grid == "blocks":
            grid = re.findall(r"const unsigned blocks = (\w+\()", api[:at])[-1]
        assert grid.startswith(rule), (row["kernel"], grid)


def test_every_loop_of_the_headers_has_a_row():
    """What `for \\(.*\\+= ?(W|stride)` finds in the nine headers, kernel by kernel, is what the inventory lists, under the rule it names: a
    step of 4 x gridDim.x wavefronts is the persistent rule's, one of 256 x gridDim.x lanes the lane rule's.  The same for vr_comp.h."""
    found = [(h, k, per) for h in lc.HEADERS for k, _, per in loops_of(h)]
    assert [(h, k) for h, k, _ in found] == [(r["header"], r["kernel"]) for r in lc.ROWS]
    assert len(found) == 22
    for (h, k, per), row in zip(found, lc.ROWS):
        assert per == {"tool": 4, "lane": 256}[row["rule"]], (h, k, per)
        assert row["carries"] and row["collective"] and row["counts"] and (row["case"] or row["existing"])
    comp = loops_of("vr_comp.h")
    assert [(k, {4: "tool", 256: "lane"}[per]) for k, _, per in comp] == [(k, rule) for k, rule, _, _ in lc.COMP_ROWS]
    assert all(test.startswith("test_") for _, _, _, test in lc.COMP_ROWS)
    # a collective inside a loop sits in a kernel whose row says why its trip count is uniform
    for header in lc.HEADERS:
        src = text(header)
        for row in (r for r in lc.ROWS if r["header"] == header):
            body = src[src.index("void " + row["kernel"] + "("):]
            body = body[:body.index("\n}\n")]
            if re.search(r"vr_ballot|wave_sum_u64|__shfl|wave_m(in|ax)_|grow_wave_or|readlane", body):
                assert len(row["collective"]) > 40 and not row["collective"].startswith("none"), row["kernel"]


def counts_of(row):
    n = row["n"]
    if n is None:  # the raster's items: both forms of both cases
        out = []
        for name in lc.RASTER_PER_SLICE:
            _, lo, hi = lc.WORD_BOXES[name]
            points, polygons = lc.raster_polygons(name)
            out += [lc.raster_items(points, polygons, rc.GRIDS[1], lo, hi, plain)[0] for plain in (False, True)]
        points, polygons = lc.raster_exact_polygons()
        out += [lc.raster_items(points, polygons, rc.GRIDS[1], *lc.RASTER_EXACT[1:], plain)[0] for plain in (False, True)]
        return out
    return list(n) if isinstance(n, tuple) else [n]


def test_every_case_goes_round_again_and_ends_in_a_partial_pass():
    for row in lc.ROWS:
        for n in counts_of(row):
            rounds, tail, per = lc.passes(row["rule"], n)
            assert rounds >= 2 and 0 < tail < per, (row["kernel"], n, rounds, tail)
            assert per == (lc.WORDS_PER_PASS if row["rule"] == "tool" else lc.LANE_CAP)
    exact = 2 * lc.WORDS_PER_PASS + 1
    assert lc.WX == lc.UX == exact == lc.MESH_WORDS[1] == lc.RESAMPLE_UNITS[1]
    for row in lc.ROWS:  # the persistent rule: a box of exactly two passes and one
        if row["rule"] == "tool":
            assert exact in counts_of(row), row["kernel"]
    assert counts_of(lc.ROWS[4])[-2:] == [exact, exact] and lc.ROWS[4]["kernel"] == "raster_rows_kernel"  # (one item a polygon in both forms)
    # the counts are those of the cases
    assert (lc.W1, lc.W3, lc.WX) == tuple(lc.box_words(lo, hi) for _, lo, hi in lc.WORD_BOXES.values()) == (4160, 4320, 4097)
    assert (lc.U1, lc.UX) == tuple(lc.box_units(lo, hi) for _, lo, hi in lc.UNIT_BOXES.values()) == (4352, 4097)
    for shape, lo, hi in lc.UNIT_BOXES.values():  # grow's rounds and write walk the bricks of the volume: as many as the box's units
        assert int(np.prod([(n + 3) // 4 for n in shape])) == lc.box_units(lo, hi)
    # inside the volume, and off one of its faces
    for boxes in (lc.WORD_BOXES, lc.UNIT_BOXES, lc.RESAMPLE_BOXES, lc.MESH_BOXES, {"wide": lc.WIDE_MESH, "raster": lc.RASTER_EXACT}):
        for shape, lo, hi in boxes.values():
            assert any(l > 0 or h < n for l, h, n in zip(lo, hi, shape[::-1])) and all(0 <= l < h <= n for l, h, n in zip(lo, hi, shape[::-1]))
    assert lc.MESH_WORDS == tuple(int(np.prod([(hi[0] - lo[0] + 63) // 64, hi[1] - lo[1], hi[2] - lo[2]])) for _, lo, hi in lc.MESH_BOXES.values())
    _, (x0, y0, z0), (x1, y1, z1) = lc.WIDE_MESH
    assert lc.WIDE_MESH_WORDS == tuple((x1 - x0 + 2 * c + 63) // 64 * (y1 - y0 + 2 * c) * (z1 - z0 + 2 * c) for c in (0, 1))
    assert (x1 - x0 + 63) // 64 == 3 == (x1 - x0 + 2 + 63) // 64
    nz, ny, nx = lc.ROD_SHAPE
    assert lc.ROD_WORDS == (ny * nz, (ny + 2) * (nz + 2)) and lc.VWORDS == 9 * 65535 > lc.LANE_CAP
    (x0, y0, z0), (x1, y1, z1) = lc.VWORDS_BOX
    assert lc.VWORDS == (z1 - z0) * (y1 - y0 + 1) * (lc.VWORDS_SHAPE[2] // 64 + 1) and y0 > 0


def test_set_voxels_lie_in_the_words_of_the_later_passes():
    """Density 0.3 .. 0.5 over the voxels of the words (units) from number WORDS_PER_PASS on; the raster's later items are whole
    polygons; the rod's bands hold the lattice words 2 x WORDS_PER_PASS and LANE_CAP, with and without the cap; the outline's later vertex
    words and nodes come from content of the same density as the first."""
    for name in lc.WORD_BOXES:
        a, lo, hi = lc.word_case(name)
        index = lc.word_index(a.shape, lo, hi)
        assert int(index.max()) + 1 == lc.box_words(lo, hi) and 0.3 <= lc.later_density(a, index) <= 0.5, name
        assert a[index >= index.max() - 2].any()  # (the last row of words)
        assert name != "exact_words" or a[index == 2 * lc.WORDS_PER_PASS].sum() > 5  # (the one word of the third pass)
    for name in lc.UNIT_BOXES:
        shape, lo, hi = lc.UNIT_BOXES[name]
        index = lc.unit_index(shape, lo, hi)
        assert int(index.max()) + 1 == lc.box_units(lo, hi)
        assert 0.3 <= lc.later_density(lc.seeded(shape, lc.DENSITY, 70), index) <= 0.5       # the histogram's mask
        for connectivity in (6, 26):
            import grow_ref as gr
            v, vlo, vhi, seeds, _, _ = lc.grow_case(name, connectivity)
            q = gr.qualifies(v[..., 3], vlo, vhi, lo, hi)
            assert 0.3 <= lc.later_density(q, index) <= 0.5 and len(seeds) == 64, (name, connectivity)
    for name in lc.RASTER_PER_SLICE:
        shape, lo, hi = lc.WORD_BOXES[name]
        points, polygons = lc.raster_polygons(name)
        for plain in (False, True):
            n, spans = lc.raster_items(points, polygons, rc.GRIDS[1], lo, hi, plain)
            later = [p for p, s in zip(polygons, spans) if s and s[0] >= lc.WORDS_PER_PASS]
            assert len(later) >= 40 and {p[3] for p in later} == {0, 1} and all(p[1] == 11 for p in later), (name, plain, n)
    # the rod
    v, bands = lc.rod()
    has = (v >= lc.ROD_LEVEL).any(axis=(1, 2))
    assert [(a, b) for a, b in lc.content_bands(v, lc.ROD_LEVEL, (0, 0, 0), lc.ROD_SHAPE[::-1])] == bands and len(bands) == 6
    for cap, per_slice in ((0, 9), (1, 11)):
        for word in (2 * lc.WORDS_PER_PASS, lc.LANE_CAP):
            z = word // per_slice - cap  # the slice of voxels that lattice word `word` lies in
            assert has[z - 3:z + 4].all(), (cap, word)
    assert has[0] and has[-1] and 0.3 <= float((v[bands[3][0]:bands[3][1]] >= lc.ROD_LEVEL).mean()) <= 0.5
    # the mesh's rows of three words: a band around the slices of the lattice words WORDS_PER_PASS and 2 x WORDS_PER_PASS
    w, wbands = lc.wide_mesh()
    _, wlo, whi = lc.WIDE_MESH
    whas = (w[:, wlo[1]:whi[1], wlo[0]:whi[0]] >= lc.MESH_LEVEL).any(axis=(1, 2))
    assert lc.content_bands(w, lc.MESH_LEVEL, wlo, whi) == wbands
    for cap, per_slice in ((0, 15), (1, 21)):
        for word in (lc.WORDS_PER_PASS, 2 * lc.WORDS_PER_PASS):
            z = word // per_slice - cap
            assert whas[z - 1:z + 2].all(), (cap, word)
    assert all(0.3 <= float((w[a:b, wlo[1]:whi[1], wlo[0]:whi[0]] >= lc.MESH_LEVEL).mean()) <= 0.5 for a, b in wbands)
    # the outlines
    m = lc.vwords_members()
    rows_first = lc.LANE_CAP // 9  # vertex rows per slice of the first pass's share ... the later words are the later slices' rows
    assert 0.3 <= float(m[0, 8].mean()) <= 0.5 and 0.3 <= float(m[0, :, rows_first:].mean()) <= 0.5
    for name, nodes in (("board_split", lc.BOARD_NODES), ("board_join", lc.BOARD_NODES), ("fish", lc.FISH_NODES)):
        assert trace(name)[1]["result"][0] == nodes > lc.LANE_CAP, name


def test_the_lattice_queues_more_bricks_than_wavefronts():
    """The frontier form's queue, round by round, counted over Q's brick adjacency: 64 disjoint octahedral shells, 2432 bricks in round
    4.  A brick that no listed brick has reached before has R = 0, so the first that reaches it queues it: the kernel's list of a round
    holds at least the round's shell.  Every brick's own ten voxels of Q are connected and every seed is one of them."""
    import grow_ref as gr
    v, seeds = lc.lattice_case()
    q = gr.qualifies(v[..., 3], *lc.LATTICE_WINDOW, (0, 0, 0), lc.LATTICE_SHAPE[::-1])
    bricks = q.reshape(32, 4, 32, 4, 32, 4).transpose(0, 2, 4, 1, 3, 5).reshape(-1, 4, 4, 4)
    tripod = np.zeros((4, 4, 4), bool)
    tripod[0, 0, :] = tripod[0, :, 0] = tripod[:, 0, 0] = True
    assert (bricks == tripod).all() and len(seeds) == 64 and all(q[z, y, x] and x % 4 == y % 4 == z % 4 == 0 for x, y, z in seeds)
    shells = lc.frontier_shells(q, seeds, 4)
    assert shells == [64 * (4 * k * k + 2) if k else 64 for k in range(4)] and shells[3] == lc.LATTICE_QUEUE > lc.WORDS_PER_PASS
    assert all(n <= lc.WORDS_PER_PASS for n in shells[:3])


def test_the_fishbone_is_one_loop():
    """One 4-connected piece without a hole has one outline; the restatement finds it, longer than LANE_CAP, and needs every round.  A
    small fishbone is walked crack by crack."""
    s = lc.fishbone()
    assert cr.label(s[None], cr.PLANE_FACES)[1] == 1
    assert cr.label(~np.pad(s, 1)[None], cr.PLANE_ALL)[1] == 1  # the outside, with the frame around the slice: no hole
    m, want = trace("fish")
    assert want["result"][1] == 1 and want["longest"] == want["result"][0] == lc.FISH_NODES > lc.LANE_CAP
    assert want["rounds"] == 20 and (1 << 19) < lc.FISH_NODES <= (1 << 20)
    assert want["result"][4][0] == 2 * int(s.sum())  # (SPLIT, unit spacing: half the shoelace sum is the member count)
    small = lc.fishbone(9, 13)
    loops = oc.walk(small, orf.SPLIT)
    ms = np.zeros((4, 1, 9, 13), bool)
    ms[0, 0] = small
    got = orf.trace(ms, 1, orf.SPLIT, (0, 0, 0), (13, 9, 1))
    assert len(loops) == 1 and got["result"][:2] == (len(loops[0]), 1) and got["points"].tolist() == [list(p) for p in loops[0]]
    board = trace("board_split")[1]
    assert board["result"][1] == 520 * 520 // 2 and board["result"][4][0] == 520 * 520


def same_mesh(got, want):
    return (got["result"] == want["result"] and np.array_equal(got["vertices"].view(np.uint32), want["vertices"].view(np.uint32))
            and np.array_equal(got["triangles"], want["triangles"]) and got["edges"] == want["edges"]
            and got["vertices"].dtype == want["vertices"].dtype and got["triangles"].dtype == want["triangles"].dtype)


SWEEP = mcs.sweep(40)


@pytest.mark.parametrize("i", range(40))
def test_banded_mesh_reference_on_the_sweep(i):
    c = SWEEP[i]
    want = mr.extract(c["v"], c["level"], c["cap"], c["box_lo"], c["box_hi"])
    assert same_mesh(lc.banded_extract(c["v"], c["level"], c["cap"], c["box_lo"], c["box_hi"], mr.extract), want), c["seed"]


@pytest.mark.parametrize("cap", [0, 1])
def test_banded_mesh_reference_on_two_bands(cap):
    """9 x 8 x 150 voxels (11 200 cells without the cap), content in slices 0 .. 11 and 120 .. 149, in a box that cuts the first band
    and ends with the second: the assembled mesh is mesh_ref.extract's, and its counts mesh_ref.counts'."""
    rng = np.random.default_rng(91)
    v = np.zeros((150, 8, 9), np.float32)
    v[:12] = rng.random((12, 8, 9))
    v[120:] = rng.random((30, 8, 9))
    lo, hi = (1, 0, 3), (9, 8, 150)
    assert lc.content_bands(v, 0.5, lo, hi) == [(3, 12), (120, 150)]
    want = mr.extract(v, 0.5, cap, lo, hi)
    got = lc.banded_extract(v, 0.5, cap, lo, hi, mr.extract)
    assert same_mesh(got, want) and want["result"][1] > 1000 and want["result"][:4] == mr.counts(v, 0.5, cap, lo, hi)
    assert not cap or mr.is_closed(got["triangles"])


def test_the_rod_reference_counts():
    v, _ = lc.rod()
    lo, hi = (0, 0, 0), lc.ROD_SHAPE[::-1]
    for cap in (0, 1):
        got = lc.banded_extract(v, lc.ROD_LEVEL, cap, lo, hi, mr.extract)
        assert got["result"][:4] == mr.counts(v, lc.ROD_LEVEL, cap, lo, hi) and got["result"][1] > 1000
        assert got["result"][5][2] == 65535 - 1 + cap and got["result"][4][2] == -cap


# ---- the channel tools: vr_filter.h, vr_rank.h, vr_gamma.h -------------------------------------------------------------------------------

def channel_loops(header):
    """[(kernel, rule)] of every grid-stride loop of a channel tool's header, in order: a tile loop steps by gridDim.x, a lane loop by
    `step`, which its kernel sets to 256 x gridDim.x."""
    out, kernel, has_step = [], None, False
    for line in text(header).splitlines():
        m = re.search(r"__global__.* void (\w+)\(", line)
        if m:
            kernel, has_step = m.group(1), False
        has_step = has_step or bool(re.search(lc.LANE_STEP, line))
        if re.search(lc.TILE_LOOP, line):
            out.append((kernel, "tile"))
        elif re.search(lc.LANE_LOOP, line):
            assert has_step, kernel
            out.append((kernel, "lane"))
        else:
            assert not re.search(r"for \(.*\+= ?(gridDim|step|stride|W)\b", line), (kernel, line)  # (no grid-stride loop of another shape)
    return out


def test_every_loop_of_the_channel_tools_has_a_row():
    found = [(h, k, rule) for h in lc.CHANNEL_HEADERS for k, rule in channel_loops(h)]
    assert found == [(h, k, rule) for h, k, rule, _, _ in lc.CHANNEL_ROWS] and len(found) == 10
    for header in lc.CHANNEL_HEADERS:  # one loop per kernel, and no kernel without one
        kernels = re.findall(r"__global__.* void (\w+)\(", text(header))
        assert kernels == [k for h, k, _ in found if h == header], header
    for header, kernel, rule, counts, test in lc.CHANNEL_ROWS:
        api = text(lc.CHANNEL_API[header])
        launches = list(re.finditer(r"hipLaunchKernelGGL\(\(?" + kernel + r"\b(?:<[^>]*>)?\)?, (.*?), dim3\(256\)", api))
        assert launches, kernel
        for m in launches:
            grid, at = m.group(1), m.start()
            if "blocks" in grid and "lane_blocks(" not in grid:  # a grid computed on an earlier line
                grid = re.findall(r"(?:const unsigned blocks = |const dim3 blocks\()(\w+\()", api[:at])[-1]
            assert "lane_blocks(" in grid, (kernel, grid)
        module, name = test.split(".")
        with open(os.path.join(ROOT, "tests", module + ".py")) as f:
            assert re.search(r"^def " + name + r"\(", f.read(), re.M), test
        assert counts


def test_the_filter_case_goes_round_in_every_loop():
    """The tiles and voxels of tests/loop_cases.py's filter case from the tile constants of csrc/vr_filter.h and the launch rule, each
    past the 2048 workgroups or the 524 288 lanes of one trip with a partial last trip; and the tail of the volume, which the write
    reaches on its second trip alone, decides all three result words."""
    import filter_ref as fr
    src = text("vr_filter.h")
    run, rows, t = (int(re.search(r"constexpr int %s = (\d+);" % k, src).group(1)) for k in ("kFilterRun", "kFilterRows", "kFilterT"))
    nz, ny, nx = lc.FILTER_ROUND_SHAPE
    tiles = (-(-nx // run) * -(-(ny * nz) // rows), -(-nx // 64) * -(-ny // t) * nz, -(-nx // 64) * -(-nz // t) * ny)
    assert tiles == lc.FILTER_ROUND_TILES and nx * ny * nz == lc.FILTER_ROUND_VOXELS
    for n in tiles:
        assert lc.lane_blocks(256 * n) == 4 * lc.TOOL_BLOCKS < n and n % (4 * lc.TOOL_BLOCKS)
    assert lc.passes("lane", lc.FILTER_ROUND_VOXELS)[:2] == (2, lc.FILTER_ROUND_VOXELS - lc.LANE_CAP)
    assert lc.FILTER_ROUND_VOXELS - lc.FILTER_ROUND_TAIL >= lc.LANE_CAP
    a, b = lc.filter_round_case()
    w = np.random.default_rng(102).normal(0.0, 0.3, 5).astype(np.float32)  # (test_filter_gpu's G[2])
    out, res, _ = fr.filter(a, None, 3, 0, (w, w, w))
    _, other, _ = fr.filter(b, None, 3, 0, (w, w, w))
    assert res[1] > 0 and other[1] == 0 and res[2] != other[2] and res[3] != other[3]
    head = out[..., 0].reshape(-1)[:lc.LANE_CAP]  # the first trip's voxels hold neither a NaN nor the extremes
    assert np.isfinite(head).all() and fr.key(head).min() > fr.key(np.array([res[2]], np.uint32).view(np.float32))[0]
    assert fr.key(head).max() < fr.key(np.array([res[3]], np.uint32).view(np.float32))[0]
