"""The voxel tools where their launch loops go round again (tests/loop_cases.py has the inventory and the cases, tests/test_loop_passes.py
checks on the CPU that every case passes its threshold with content in the later passes): boxes of 4160, 4320 and exactly
2 x WORDS_PER_PASS + 1 words or units for the persistent kernels, more than LANE_CAP vertex words, nodes, corners of one loop and lattice
words for the kernels with one lane per element.  Everything EQUAL to the numpy restatements, through the checks of each tool's own GPU
tests, in both kernel forms."""
import numpy as np
import pytest

import comp_cases as cc
import dist_cases as dc
import loop_cases as lc
import mesh_ref as mr
import morph_cases as mc
import morph_ref as mor
import outline_cases as oc
import raster_cases as rc
import resample_cases as rsc
import test_components_scale_gpu as tcs
import test_distance_gpu as tdg
import test_grow_gpu as tgg
import test_histogram_gpu as thg
import test_mesh_gpu as tmg
import test_morph_gpu as tmo
import test_outline_gpu as tog
import test_raster_gpu as trg
import test_resample_gpu as trs
from volumerendering_amd import capi

pytestmark = pytest.mark.gpu
f32 = np.float32
W, H = 64, 48
WORD_NAMES = list(lc.WORD_BOXES)


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(W, H, 0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def defaults(ctx):
    yield
    ctx.set_kernel_flavour(0)
    ctx.set_volume_layout(0)
    ctx.set_arithmetic(capi.ARITH_SEPARATE)


# ---- persistent rule, words ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", WORD_NAMES)
def test_morph_over_more_words_than_wavefronts(ctx, name):
    """bit_pack_kernel and morph_write_kernel: |A'|, |R| and their boxes are a wavefront's sums over two or three words.  NONE stores the
    pack as it is; CLOSE runs both dilations between; OR keeps the destination's arbitrary bits where R is not."""
    a, lo, hi = lc.word_case(name)
    shape = a.shape
    src = mc.hostile(a, 2, seed=62)
    state = mc.arbitrary_bits(shape, seed=63)
    ctx.volume_upload(0, src)
    ctx.volume_upload(1, state)
    for op, combine in ((capi.MORPH_NONE, capi.MORPH_REPLACE), (capi.MORPH_CLOSE, capi.MORPH_OR), (capi.MORPH_ERODE, capi.MORPH_ANDNOT)):
        for flavour in (0, 1):
            ctx.set_kernel_flavour(flavour)
            d = tmo.desc(shape, op, mor.ball((1, 1, 1), 1), (lo, hi), src_contour=2, dst_contour=op % 4, combine=combine)
            res, _, state, _ = tmo.check(ctx, d, src, state, what=(name, op, flavour))
            assert res.src_voxels > 0.3 * lc.WORDS_PER_PASS * 64


@pytest.mark.parametrize("name", WORD_NAMES)
def test_distance_over_more_words_than_wavefronts(ctx, name):
    """dist_x_kernel over every word of both fields and dist_write_kernel with a probe: the voxels beyond the limit, the probe's count,
    minimum and maximum are a wavefront's over two or three words."""
    a, lo, hi = lc.word_case(name)
    shape = a.shape
    src = mc.hostile(a, 0, seed=64)
    state = mc.hostile(lc.seeded(shape, 0.3, 65), 1, seed=66)  # the destination, and the probe in its contour 1
    ctx.volume_upload(0, src)
    ctx.volume_upload(1, state)
    for mode, limit in ((capi.DIST_SIGNED, 0), (capi.DIST_OUTSIDE, 1500), (capi.DIST_INSIDE, 0)):
        for flavour in (0, 1):
            ctx.set_kernel_flavour(flavour)
            probe = mode != capi.DIST_INSIDE
            d = tdg.desc(shape, mode, (lo, hi), dst_channel=2 + (mode == capi.DIST_INSIDE), spacing=dc.MM, limit=limit,
                         probe_slot=1 if probe else -1, probe_contour=1)
            res, cnt, after = tdg.check(ctx, d, src, state, probe=state if probe else None, what=(name, mode, flavour))
            if probe:
                assert res.probe_voxels > 0.2 * lc.WORDS_PER_PASS * 64
            if limit:
                assert res.beyond > 0
            if flavour == 1 or mode != capi.DIST_INSIDE and not limit:
                assert cnt[1] == cnt[0]  # the x pass took every word of the box
            state = after


@pytest.mark.parametrize("name", ["one_word", "three_words"])
def test_raster_over_more_items_and_words_than_wavefronts(ctx, name):
    """raster_rows_kernel over more than WORDS_PER_PASS items in both forms, raster_write_kernel over the box's words: two contours,
    both rules."""
    shape, lo, hi = lc.WORD_BOXES[name]
    grid = rc.GRIDS[1]
    points, polygons = lc.raster_polygons(name, grid)
    ctx.volume_upload(0, np.zeros(shape + (4,), f32))
    state = mc.arbitrary_bits(shape, seed=67)
    ctx.volume_upload(1, state)
    for rule in (capi.POLY_EVEN_ODD, capi.POLY_UNION):
        for flavour in (0, 1):
            assert lc.raster_items(points, polygons, grid, lo, hi, bool(flavour))[0] > lc.WORDS_PER_PASS
            ctx.set_kernel_flavour(flavour)
            d = trg.desc(shape, grid, (lo, hi), contours=0b0011, rule=rule, combine=(capi.MORPH_REPLACE, capi.MORPH_OR)[rule])
            res, _, state, r = trg.check(ctx, d, points, polygons, shape, state, what=(name, rule, flavour))
            assert r[0, hi[2] - 1].any() and r[1, hi[2] - 1].any()  # (the last slice's polygons are the last items)


def test_raster_write_over_exactly_two_passes_and_a_word(ctx):
    shape, lo, hi = lc.WORD_BOXES["exact_words"]
    grid = rc.GRIDS[1]
    polys = [(rc.place(rc.ngon(9, 20, 9 + z % 2, 17, 8.2, phase=0.2 * z), grid[1], grid[0]), z, z % 2) for z in range(shape[0])]
    points, polygons = rc.flatten(polys)
    ctx.volume_upload(0, np.zeros(shape + (4,), f32))
    state = mc.arbitrary_bits(shape, seed=68)
    ctx.volume_upload(1, state)
    for flavour in (0, 1):
        ctx.set_kernel_flavour(flavour)
        d = trg.desc(shape, grid, (lo, hi), contours=0b0011, combine=capi.MORPH_AND)
        res, _, state, r = trg.check(ctx, d, points, polygons, shape, state, what=flavour)
        assert r[(hi[2] - 1) % 2, hi[2] - 1].any()


# ---- persistent rule, units ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(lc.UNIT_BOXES))
def test_histogram_with_a_mask_over_more_units_than_wavefronts(ctx, name):
    """All five rows (test_histogram_gpu.test_large_volume_many_blocks has row 0 alone at this size): the private copy in LDS and the
    per-lane row sums collect over two or three units per wavefront; 4096 bins x 5 rows go straight to global memory."""
    shape, lo, hi = lc.UNIT_BOXES[name]
    v = thg.noise(shape, seed=69)
    m = mc.hostile(lc.seeded(shape, lc.DENSITY, 70), 1, seed=71)
    ctx.volume_upload(0, v)
    ctx.volume_upload(1, m)
    for bins, policy in ((256, capi.HIST_CLAMP), (4096, capi.HIST_DROP)):
        for flavour in (0, 1):
            ctx.set_kernel_flavour(flavour)
            for channel in (3, 0):
                thg.check(ctx, thg.desc(shape, (lo, hi), bins=bins, scale=float(bins) * 0.9, out_of_range=policy, mask_slot=1, rows=0b11111,
                                        channel=channel), v, m, what=(name, bins, flavour, channel))
            thg.check(ctx, thg.desc(shape, (lo, hi), bins=bins, scale=float(bins), out_of_range=policy), v, what=(name, bins, flavour, "unmasked"))


@pytest.mark.parametrize("connectivity", [capi.GROW_FACES, capi.GROW_ALL])
@pytest.mark.parametrize("name", list(lc.UNIT_BOXES))
def test_grow_over_more_units_and_bricks_than_wavefronts(ctx, name, connectivity):
    """grow_classify_kernel over the box's units, grow_round_kernel (the sweep form: every brick, every round) and grow_write_kernel over
    the volume's bricks; REPLACE into a mask of arbitrary bits stores zeros too."""
    v, vlo, vhi, seeds, lo, hi = lc.grow_case(name, connectivity)
    shape = v.shape[:3]
    state = mc.arbitrary_bits(shape, seed=72)
    ctx.volume_upload(0, v)
    ctx.volume_upload(1, state)
    for flavour in (0, 1):
        ctx.set_kernel_flavour(flavour)
        res, cnt, state, r, q = tgg.check(ctx, tgg.desc(shape, seeds, vlo, vhi, connectivity, (lo, hi), contour=flavour), v, state,
                                          what=(name, connectivity, flavour))
        assert res.voxels > 0.1 * lc.WORDS_PER_PASS * 64 and lc.later_density(r, lc.unit_index(shape, lo, hi)) > 0.1


def test_grow_frontier_of_more_bricks_than_wavefronts(ctx):
    """The frontier form of grow_round_kernel with 2432 bricks queued for round 4 (loop_cases.lattice_case; test_loop_passes.py counts
    the queues): list_in[i] for i >= W.  Everything of Q is reached; the sweep form agrees."""
    v, seeds = lc.lattice_case()
    shape = lc.LATTICE_SHAPE
    state = np.zeros(shape + (4,), f32)
    ctx.volume_upload(0, v)
    ctx.volume_upload(1, state)
    for flavour in (0, 1):
        ctx.set_kernel_flavour(flavour)
        d = tgg.desc(shape, seeds, *lc.LATTICE_WINDOW, capi.GROW_FACES, contour=1 + flavour)
        res, cnt, state, r, q = tgg.check(ctx, d, v, state, what=flavour)
        assert res.voxels == int(q.sum()) == 10 * 32 ** 3 and res.rounds > 4


def test_raster_of_exactly_two_passes_and_an_item(ctx):
    """raster_rows_kernel over 2 x WORDS_PER_PASS + 1 items in either form: 4097 small polygons of one item each."""
    shape, lo, hi = lc.RASTER_EXACT
    grid = rc.GRIDS[1]
    points, polygons = lc.raster_exact_polygons(grid)
    ctx.volume_upload(0, np.zeros(shape + (4,), f32))
    state = mc.arbitrary_bits(shape, seed=86)
    ctx.volume_upload(1, state)
    for flavour in (0, 1):
        assert lc.raster_items(points, polygons, grid, lo, hi, bool(flavour))[0] == 2 * lc.WORDS_PER_PASS + 1
        ctx.set_kernel_flavour(flavour)
        d = trg.desc(shape, grid, (lo, hi), contours=0b0011, rule=flavour, combine=capi.MORPH_REPLACE)
        res, _, state, r = trg.check(ctx, d, points, polygons, shape, state, what=flavour)
        assert r[0, hi[2] - 1].any() and r[1, hi[2] - 1].any()


@pytest.mark.parametrize("name", list(lc.RESAMPLE_BOXES))
def test_resample_over_more_units_than_wavefronts(ctx, name):
    """resample_kernel's walk advances (row, piece) by stride / ux and stride % ux with a carry: three passes of it, in the three forms
    (plain, default, density alone) and both filters; the inside count, its box and the loaded voxels are a wavefront's over its units."""
    shape, lo, hi = lc.RESAMPLE_BOXES[name]
    src_shape = rsc.SRC_SHAPES[0]
    src = rsc.hostile(src_shape, 73)
    ctx.volume_upload(0, src)
    state = rsc.arbitrary_bits(shape, 74)
    ctx.volume_upload(1, state)
    geom = rsc.transform("rot30z", src_shape, shape)
    assert lc.resample_units(lo, hi) > 2 * lc.WORDS_PER_PASS
    for channels, filt in ((15, capi.RESAMPLE_LINEAR), (8, capi.RESAMPLE_LINEAR), (5, capi.RESAMPLE_NEAREST)):
        for flavour in (0, 1):
            ctx.set_kernel_flavour(flavour)
            d = trs.desc(shape, geom, (lo, hi), channels=channels, filter=filt)
            res, _, state, want = trs.check(ctx, d, src, state, fused=bool(flavour), what=(name, channels, filt, flavour))
            assert want[0] > 10000 and want[1] > 10000  # (voxels inside and outside)


# ---- lane rule: the outlines ---------------------------------------------------------------------------------------------------------

def areas_are_the_member_counts(res, m, d):
    """SPLIT at unit spacing: every loop of a contour is the boundary of a 4-connected piece or of a hole in one, so half the summed
    shoelace terms is the number of members in the box -- whatever the restatement says."""
    want = lc.member_counts(m, d.contours, tuple(d.box_lo), tuple(d.box_hi))
    assert all(a % 2 == 0 for a in res.area2) and tuple(a // 2 for a in res.area2) == want, (tuple(res.area2), want)


def outline_both_forms(ctx, d, m, what):
    """One call in the default form against the restatement, the plain form's output equal to it and its rounds the fixed count."""
    want = tog.reference(d, m)
    ctx.set_kernel_flavour(0)
    a_pts, a_polys, a_res, a_cnt, _ = tog.check(ctx, d, m, what=(what, 0), want=want)
    assert a_cnt[2] == want["rounds"], (what, a_cnt, want["rounds"])
    ctx.set_kernel_flavour(1)
    b_pts, b_polys, b_res, b_cnt, _ = tog.check(ctx, d, m, what=(what, 1), want=want)
    assert b_cnt[2] == int(np.ceil(np.log2(b_cnt[0]))), (what, b_cnt)
    return want, a_res


def test_outline_more_vertex_words_than_lanes(ctx):
    """outline_corners_kernel: 589 815 vertex words of one contour, one word a vertex row (the restatement takes 7 s: its arrays have 64
    columns whatever the row holds)."""
    m = lc.vwords_members()
    ctx.volume_upload(0, oc.volume(m, seed=75))
    d = tog.desc(lc.VWORDS_SHAPE, box=lc.VWORDS_BOX)
    want, res = outline_both_forms(ctx, d, m, "vertex words")
    assert want["result"][0] > lc.LANE_CAP
    areas_are_the_member_counts(res, m, d)


@pytest.mark.parametrize("connect", [capi.OUTLINE_SPLIT, capi.OUTLINE_JOIN], ids=["split", "join"])
def test_outline_more_nodes_than_lanes(ctx, connect):
    """A checkerboard slice: every interior vertex is a saddle, 540 800 nodes.  SPLIT: every voxel on its own; JOIN: diagonal chains."""
    m = lc.board_members()
    ctx.volume_upload(0, oc.volume(m, seed=76))
    d = tog.desc(lc.BOARD_SHAPE, oc.GRIDS[2], None, (250, 699), connect=connect)
    want, res = outline_both_forms(ctx, d, m, ("checkerboard", connect))
    assert want["result"][0] == lc.BOARD_NODES > lc.LANE_CAP
    if connect == capi.OUTLINE_SPLIT:
        assert res.n_polygons == 520 * 520 // 2
        unit = tog.desc(lc.BOARD_SHAPE)
        ctx.set_kernel_flavour(0)
        areas_are_the_member_counts(ctx.mask_outlines(unit)[2], m, unit)


def test_outline_one_loop_of_more_corners_than_lanes(ctx):
    """The fishbone: ONE loop of 610 984 corners.  Every doubling round changes something, so the default form runs all 20 as the plain
    one does, with windows up to 2^19 and every lane's `any` spanning two nodes."""
    m = lc.fishbone_members()
    ctx.volume_upload(0, oc.volume(m, seed=77))
    d = tog.desc(lc.FISH_SHAPE)
    want, res = outline_both_forms(ctx, d, m, "fishbone")
    assert want["longest"] == want["result"][0] == lc.FISH_NODES > lc.LANE_CAP and res.n_polygons == 1
    assert want["rounds"] == 20 == int(np.ceil(np.log2(lc.FISH_NODES)))
    areas_are_the_member_counts(res, m, d)


def test_components_of_the_background(ctx):
    """comp_complement_kernel over more than LANE_CAP box words: the background of the vertex-word case's set, 8-connected in its
    one-voxel-wide slices (runs along y), the three largest kept."""
    a = lc.vwords_members()[0]
    shape = a.shape
    lo, hi = lc.VWORDS_BOX
    src = cc.volume(a, 1, seed=78)
    state = mc.arbitrary_bits(shape, seed=79)
    ctx.volume_upload(0, src)
    ctx.volume_upload(1, state)
    d = tcs.desc(shape, box=(lo, hi), src_contour=1, background=1, connectivity=capi.COMP_ALL, keep_largest=3,
                 dst_slot=1, dst_contour=0, label_slot=1, label_channel=3)
    want = cc.reference_arrays(src, state, 1, 1, d.connectivity, lo, hi, keep_largest=3, dst_contour=0, label_channel=3)
    assert cc.box_words(shape, lo, hi) > lc.LANE_CAP
    tcs.check_arrays(ctx, d, want, shape, what="background")


# ---- the mesh ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(lc.MESH_BOXES))
def test_mesh_over_more_lattice_words_than_wavefronts(ctx, name):
    """mesh_pack_kernel, mesh_vertex_kernel and mesh_triangle_kernel over 4160 and 4097 lattice words of noise: vertices bit for bit,
    triangles, result and counters."""
    shape, lo, hi = lc.MESH_BOXES[name]
    v = lc.mesh_values(name)
    ctx.volume_upload(0, tmg.mc.vec4(v, 3, seed=80))
    d = tmg.desc(shape, lc.MESH_LEVEL, 0, box=(lo, hi))
    want = mr.extract(v, d.level, 0, lo, hi)
    assert want["result"][1] > lc.WORDS_PER_PASS and want["result"][:4] == mr.counts(v, d.level, 0, lo, hi)
    for flavour in (0, 1):
        ctx.set_kernel_flavour(flavour)
        tmg.check(ctx, d, v, (name, flavour), want)


@pytest.mark.parametrize("cap", [0, 1])
def test_mesh_rows_of_three_words_over_more_lattice_words_than_wavefronts(ctx, cap):
    """mesh_pack_kernel, mesh_vertex_kernel and mesh_triangle_kernel with three words a lattice row (the triangle kernel's corners reach
    into the next word, row and slice) at u >= W: 4140 lattice words, 5838 with the cap, content in five thin bands that hold the words
    WORDS_PER_PASS and 2 x WORDS_PER_PASS.  The reference is banded_extract's, held to mesh_ref.counts as the rod's."""
    shape, lo, hi = lc.WIDE_MESH
    v, bands = lc.wide_mesh()
    ctx.volume_upload(0, tmg.mc.vec4(v, 3, seed=84))
    d = tmg.desc(shape, lc.MESH_LEVEL, cap, box=(lo, hi))
    want = lc.banded_extract(v, d.level, cap, lo, hi, mr.extract)
    assert want["result"][:4] == mr.counts(v, d.level, cap, lo, hi) and want["result"][1] > 10 * lc.WORDS_PER_PASS
    for flavour in (0, 1):
        ctx.set_kernel_flavour(flavour)
        tmg.check(ctx, d, v, (cap, flavour), want)


@pytest.mark.parametrize("cap", [0, 1])
def test_mesh_rod_more_lattice_words_than_lanes(ctx, cap):
    """mesh_count_kernel: 589 815 lattice words (720 907 with the cap) along z, content in six bands at both ends and around the words
    2 x WORDS_PER_PASS and LANE_CAP.  The reference is assembled band by band (loop_cases.banded_extract, pinned to mesh_ref.extract by
    tests/test_loop_passes.py); the whole call is held to mesh_ref.counts as well."""
    v, bands = lc.rod()
    lo, hi = tmg.whole(lc.ROD_SHAPE)
    ctx.volume_upload(0, tmg.mc.vec4(v, 3, seed=82))
    d = tmg.desc(lc.ROD_SHAPE, lc.ROD_LEVEL, cap)
    want = lc.banded_extract(v, d.level, cap, lo, hi, mr.extract)
    assert want["result"][:4] == mr.counts(v, d.level, cap, lo, hi) and want["result"][1] > 1000
    for flavour in (0, 1):
        ctx.set_kernel_flavour(flavour)
        tmg.check(ctx, d, v, (cap, flavour), want)
