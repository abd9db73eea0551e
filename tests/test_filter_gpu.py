"""The separable filters on the device (vr_volume_filter, include/vr.h) against the numpy restatement (filter_ref.py): the downloaded
destination bit for bit -- where the restatement holds a NaN that a pass computed, any NaN passes -- the result struct and all three
counters, in both kernel forms (flavour 0: LDS tiles; flavour 1: plain) and in the volume layouts 0 and 3.

The default form's tile extents (csrc/vr_filter.h): the x pass takes runs of 256 outputs of a row; the y and z passes take 64 consecutive x
by 64 outputs along the axis.  EDGE_SHAPES holds a volume one below, at and one above each of them."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import filter_ref as fr
import host_ref as hr
import index_edges_cases as ie
import loop_cases as lc
import oracle_binding as ob
import resample_cases as rc
import vrtest as vt
from volumerendering_amd import capi

pytestmark = pytest.mark.gpu
f32 = np.float32
W, H = 64, 48
with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "volumerendering_amd", "csrc", "vr_filter.h")) as _f:
    HEADER = _f.read()
FORMS = [(0, 0), (1, 0), (0, 3), (1, 3)]  # (flavour, layout)
SHAPES = [(6, 9, 70), (21, 37, 130), (5, 1, 70), (9, 6, 1)]  # (nz, ny, nx)
EDGE_SHAPES = [(2, 3, 255), (2, 3, 256), (2, 3, 257), (3, 5, 63), (3, 5, 64), (3, 5, 65), (2, 63, 5), (2, 64, 5), (2, 65, 5), (63, 2, 5),
               (64, 2, 5), (65, 2, 5), (2, 130, 66), (130, 2, 66)]
G = {r: np.random.default_rng(100 + r).normal(0.0, 0.3, 2 * r + 1).astype(f32) for r in (0, 1, 2, 8, 32)}  # arbitrary weights per radius


def boxes(shape):
    """The whole volume, a box aligned to nothing, one voxel, an empty box."""
    nx, ny, nz = rc.n_of(shape)
    mid = ((nx // 3, ny // 3, nz // 3), (max(nx // 3 + 1, nx - nx // 4), max(ny // 3 + 1, ny - ny // 5), max(nz // 3 + 1, nz - nz // 3)))
    one = (nx // 2, ny // 2, nz // 2)
    return [((0, 0, 0), (nx, ny, nz)), mid, (one, tuple(v + 1 for v in one)), ((nx // 2, 0, 0), (nx // 2, ny, nz))]


def same(got, want, computed):
    """Bit-equal; where `computed` (a mask over voxels and components) and the restatement holds a NaN, any NaN."""
    eq = vt.bits(got) == vt.bits(want)
    return bool((eq | (computed & np.isnan(want) & np.isnan(got))).all())


def check(ctx, src, before, taps, sc=3, dc=0, border=capi.FILTER_CLAMP, bv=0.0, box=None, slots=(0, 1), forms=FORMS, what=None):
    """One descriptor in every form against the restatement.  src: the source slot's voxels; before: the destination's before the call
    (ignored in place: slots[0] == slots[1]).  Both slots are uploaded again for every form.  Returns the restatement's (volume, result,
    counters)."""
    shape = src.shape[:3]
    lo, hi = box if box else ((0, 0, 0), rc.n_of(shape))
    in_place = slots[0] == slots[1]
    want, want_res, want_cnt = fr.filter(src, src if in_place else before, sc, dc, taps, border, bv, lo, hi)
    computed = np.zeros(src.shape, bool)
    if any(t is not None for t in taps):
        computed[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0], dc] = True
    for flavour, layout in forms:
        ctx.set_kernel_flavour(flavour)
        ctx.set_volume_layout(layout)
        ctx.volume_upload(slots[0], src)
        if not in_place:
            ctx.volume_upload(slots[1], before)
        d = ctx.filter_whole(slots[0], sc, slots[1], dc).copy(border=border, border_value=bv, box_lo=lo, box_hi=hi)
        res = ctx.volume_filter(d, taps)
        cnt = ctx.filter_counters()
        got = ctx.volume_download(slots[1], shape)
        if not same(got, want, computed):
            bad = np.argwhere(vt.bits(got) != vt.bits(want))
            raise AssertionError((what, flavour, layout, len(bad), bad[:4], got[tuple(bad[0])], want[tuple(bad[0])]))
        assert res.as_tuple() == want_res, (what, flavour, layout, res.as_tuple(), want_res)
        assert cnt == want_cnt, (what, flavour, layout, cnt, want_cnt)
        if not in_place:
            assert np.array_equal(vt.bits(ctx.volume_download(slots[0], shape)), vt.bits(src)), (what, flavour, layout)
    return want, want_res, want_cnt


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


@pytest.mark.parametrize("shape", SHAPES, ids=["70x9x6", "130x37x21", "70x1x5", "1x6x9"])
def test_shapes_and_boxes(ctx, shape):
    """Three passes of different radii over volumes with tails on every axis, a single row and a single column; boxes aligned to nothing,
    of one voxel and empty; both borders; into a destination of arbitrary bits, whose other components and outside voxels keep theirs."""
    src = rc.volume(shape, 11)
    before = rc.arbitrary_bits(shape, 12)
    taps = (G[2], G[8], G[1])
    for k, box in enumerate(boxes(shape)):
        border, bv = ((capi.FILTER_CLAMP, 0.0), (capi.FILTER_CONSTANT, -1.75))[k % 2]
        _, res, cnt = check(ctx, src, before, taps, 3, k % 4, border, bv, box, what=(shape, box))
        assert cnt[2] == (3 if res[0] else 0)


@pytest.mark.parametrize("shape", EDGE_SHAPES, ids=lambda s: "x".join(str(v) for v in s[::-1]))
def test_tile_edges(ctx, shape):
    """One below, at and one above the x pass' run of 256, the line passes' 64 lanes along x and their 64 outputs along y and along z; two
    tiles and a tail along x and the axis at once.  Radius 2 on every axis, the whole volume and a box across the tile edge."""
    src = rc.volume(shape, 21)
    before = rc.arbitrary_bits(shape, 22)
    nx, ny, nz = rc.n_of(shape)
    taps = (G[2], G[2], G[2])
    check(ctx, src, before, taps, what=shape)
    edge = (tuple(max(0, min(n - 2, 62)) for n in (nx, ny, nz)), tuple(min(n, 67) for n in (nx, ny, nz)))
    check(ctx, src, before, taps, 1, 2, capi.FILTER_CONSTANT, 0.5, edge, forms=FORMS[:2], what=(shape, edge))


SUBSETS = [(x, y, z) for x in (0, 1) for y in (0, 1) for z in (0, 1)]


@pytest.mark.parametrize("subset", SUBSETS, ids=lambda s: "".join(a for a, on in zip("xyz", s) if on) or "copy")
def test_every_subset_of_the_passes(ctx, subset):
    """Every subset of the three passes, the empty one included: a pure copy, bits unchanged (a NaN's payload too)."""
    shape = (6, 9, 70)
    src = rc.hostile(shape, 31)
    src.view(np.uint32)[0, 0, :4, 3] = [0x7FC12345, 0xFFC00001, 0x7F800001, 0x00000001]
    before = rc.arbitrary_bits(shape, 32)
    taps = tuple(G[r] if on else None for r, on in zip((8, 1, 2), subset))
    for border, bv in ((capi.FILTER_CLAMP, 0.0), (capi.FILTER_CONSTANT, 2.5)):
        want, res, cnt = check(ctx, src, before, taps, 3, 1, border, bv, ((1, 0, 1), (69, 9, 5)), what=(subset, border))
        assert cnt[2] == sum(subset)
    if not any(subset):
        assert np.array_equal(vt.bits(want[1:5, :, 1:69, 1]), vt.bits(src[1:5, :, 1:69, 3]))


@pytest.mark.parametrize("radii", [(0, 0, 0), (1, 1, 1), (8, 8, 8), (32, 32, 32), (32, 0, 1), (1, 32, 8), (2, 8, 32)],
                         ids=lambda r: "r" + "-".join(str(v) for v in r))
def test_radii(ctx, radii):
    """Radii 0 (one tap), 1, 8 and 32, equal and different per axis, both borders with a border_value that is not 0; the radius is larger
    than the axis for every r > 6, on 130 x 37 x 21 for 32."""
    for shape in ((5, 7, 66), (21, 37, 130)) if max(radii) == 32 else ((5, 7, 66),):
        src = rc.volume(shape, 41)
        before = rc.arbitrary_bits(shape, 42)
        taps = tuple(G[r] for r in radii)
        check(ctx, src, before, taps, 3, 0, capi.FILTER_CLAMP, 0.0, None, what=(shape, radii))
        check(ctx, src, before, taps, 2, 3, capi.FILTER_CONSTANT, -3.25, boxes(shape)[1], forms=FORMS[:2], what=(shape, radii, "constant"))


def test_a_radius_larger_than_the_axis(ctx):
    """n = 3 with r = 8 on every axis: every tap but three reads the border."""
    shape = (3, 3, 3)
    src = rc.volume(shape, 43)
    for border, bv in ((capi.FILTER_CLAMP, 0.0), (capi.FILTER_CONSTANT, 7.0)):
        check(ctx, src, rc.arbitrary_bits(shape, 44), (G[8], G[8], G[8]), 3, 3, border, bv, what=border)


def test_gaussians(ctx):
    """vr_filter_gaussian's weights, order 0 and order 1, end to end: a smoothed channel and a derivative of it."""
    shape = (21, 37, 130)
    src = rc.volume(shape, 45)
    before = rc.arbitrary_bits(shape, 46)
    g0 = [capi.filter_gaussian(s) for s in (1.0, 2.0, 2.0 / 3.0)]
    want, res, _ = check(ctx, src, before, tuple(g0), forms=FORMS[:2])
    assert res[1] == 0 and float(np.abs(want[..., 0]).max()) < float(np.abs(src[..., 3]).max())
    check(ctx, src, before, (capi.filter_gaussian(1.0, 1), g0[1], g0[2]), forms=FORMS[:2])


@pytest.mark.parametrize("shape", [(6, 9, 70), (9, 6, 1)], ids=["70x9x6", "1x6x9"])
def test_hostile_values(ctx, shape):
    """NaN, +-inf, +-0, denormals and 3e38 in the source, in the weights and as the border value; the destination of arbitrary bits."""
    src = rc.hostile(shape, 51)
    before = rc.arbitrary_bits(shape, 52)
    tiny = np.array([1e-39, -2e-40, 3e-41], f32)  # denormal weights: denormal products
    big = np.array([3e38, 1.0, -3e38], f32)
    _, res, _ = check(ctx, src, before, (G[1], G[2], G[1]), 3, 2, what="finite weights")
    assert res[1] > 0
    check(ctx, src, before, (tiny, None, tiny), 0, 0, capi.FILTER_CONSTANT, 1e-42, what="denormal")
    check(ctx, rc.volume(shape, 53) * f32(1e-38), before, (G[1], G[1], G[1]), 3, 1, what="denormal data")
    check(ctx, src, before, (big, G[1], None), 1, 3, capi.FILTER_CONSTANT, float("-inf"), what="huge")
    check(ctx, rc.volume(shape, 53), before, (np.array([1, np.nan, 1], f32), None, None), 3, 0, capi.FILTER_CONSTANT, float("nan"), forms=FORMS[:2], what="nan")
    zeros = np.where(np.random.default_rng(54).random(shape + (4,)) < 0.5, f32(0.0), f32(-0.0)).astype(f32)
    _, res, _ = check(ctx, zeros, before, (None, None, None), 3, 0, what="signed zeros")
    assert res[2:] == (0x80000000, 0)  # (-0.0f is the least value, +0.0f the greatest)
    _, res, _ = check(ctx, np.full(shape + (4,), np.nan, f32), before, (G[1], None, None), 3, 0, forms=FORMS[:2], what="all nan")
    assert res == (src[..., 0].size, src[..., 0].size, 0, 0)


def test_in_place_and_a_fresh_destination(ctx):
    """Same slot and same channel; same slot, channel 3 into channel 0; an empty destination slot is created with the source's dimensions
    and zeros, by a whole box, a partial box and an empty box."""
    shape = (21, 37, 130)
    src = rc.volume(shape, 61)
    taps = (G[8], G[2], G[8])
    check(ctx, src, None, taps, 3, 3, slots=(0, 0), what="same channel")
    check(ctx, src, None, taps, 3, 3, capi.FILTER_CONSTANT, 1.0, boxes(shape)[1], slots=(1, 1), forms=FORMS[:2], what="same channel, box")
    check(ctx, src, None, taps, 3, 0, slots=(0, 0), what="3 -> 0")
    check(ctx, src, None, (None, None, None), 2, 1, slots=(0, 0), forms=FORMS[:2], what="copy in place")
    for box in boxes(shape)[:2] + boxes(shape)[3:]:
        for flavour in (0, 1):
            with capi.Context(W, H, 0) as c:
                c.set_kernel_flavour(flavour)
                c.volume_upload(0, src)
                d = c.filter_whole(0, 3, 2, 1).copy(box_lo=box[0], box_hi=box[1])
                res = c.volume_filter(d, taps)
                want, want_res, want_cnt = fr.filter(src, None, 3, 1, taps, lo=box[0], hi=box[1])
                got = c.volume_download(2, shape)
                assert np.array_equal(vt.bits(got), vt.bits(want)) and res.as_tuple() == want_res and c.filter_counters() == want_cnt
                assert not vt.bits(got[..., [0, 2, 3]]).any()


@pytest.mark.parametrize("n", ie.RODS, ids=lambda n: "x".join(str(v) for v in n))
def test_rods(ctx, n):
    """Axes of 65535 voxels with r = 2 on every axis: 256 runs of a row, 1024 tiles along y and along z."""
    shape = (n[2], n[1], n[0])
    src = rc.volume(shape, 71)
    before = rc.arbitrary_bits(shape, 72)
    check(ctx, src, before, (G[2], G[2], G[2]), forms=FORMS[:3], what=n)
    far = tuple(max(0, v - 70) for v in n)
    check(ctx, src, before, (G[2], G[2], G[2]), 3, 1, capi.FILTER_CONSTANT, 4.0, (far, n), forms=FORMS[:2], what=(n, "far end"))


def test_the_launch_loops_go_round(ctx):
    """5 x 343 x 343 voxels with r = 2 on every axis: 14 707 tiles of the x pass, 2058 of the y pass and of the z pass for the 2048
    workgroups the default form launches at the most, 588 245 voxels for the 524 288 lanes of the plain passes and of the write.  The
    source's least and greatest value and its NaN lie in the last 50 000 voxels, which the write reaches on its second trip alone: the
    result words come out of the fold across trips."""
    src, zeroed = lc.filter_round_case()
    shape = src.shape[:3]
    nx, ny, nz = rc.n_of(shape)
    run, rows, t = (int(re.search(r"constexpr int %s = (\d+);" % k, HEADER).group(1)) for k in ("kFilterRun", "kFilterRows", "kFilterT"))
    assert -(-nx // run) * -(-(ny * nz) // rows) == lc.FILTER_ROUND_TILES[0] > lc.TOOL_BLOCKS * 4
    assert -(-nx // 64) * -(-ny // t) * nz == lc.FILTER_ROUND_TILES[1] > lc.TOOL_BLOCKS * 4
    assert -(-nx // 64) * -(-nz // t) * ny == lc.FILTER_ROUND_TILES[2] > lc.TOOL_BLOCKS * 4
    assert nx * ny * nz == lc.FILTER_ROUND_VOXELS > lc.LANE_CAP
    taps = (G[2], G[2], G[2])
    _, res, cnt = check(ctx, src, rc.arbitrary_bits(shape, 74), taps, forms=FORMS[:2], what="round again")
    other = fr.filter(zeroed, None, 3, 0, taps)[1]
    assert res[1] > 0 and other[1] == 0 and res[2] != other[2] and res[3] != other[3] and cnt == (nx * ny * nz, 3 * nx * ny * nz, 3)


def test_a_slot_of_four_gib():
    """A slot of 512 x 512 x 1032 voxels, 4.03 GiB, filtered in place from channel 3 into channel 0 with r = 1 on every axis, in a box of
    five slabs across voxel index 2^28 (the start of slab z = 1024): the box against the restatement of the slabs around it, and every
    slab near the box and every 16th slab of the rest against the source."""
    shape = (ie.A1[2], ie.A1[1], ie.A1[0])
    z0, z1 = ie.LINE_Z - 2, ie.LINE_Z + 3
    lo, hi = (100, 200, z0), (391, 263, z1)
    src = np.zeros(shape + (4,), f32)
    src[z0 - 4:z1 + 4] = rc.volume((z1 - z0 + 8, shape[1], shape[2]), 81)
    taps = (G[1], G[1], G[1])
    sub = src[z0 - 1:z1 + 1]
    want, want_res, want_cnt = fr.filter(sub, sub, 3, 0, taps, lo=(lo[0], lo[1], 1), hi=(hi[0], hi[1], 1 + z1 - z0))
    # (the restatement of a sub-volume clamps at its own z faces: slabs 0 and z1 - z0 + 1 of it, which the box does not hold and whose
    # values no voxel of the box reads through the x and y passes)
    with capi.Context(W, H, 0) as c:
        c.volume_upload(0, src)
        for flavour in (0, 1):
            c.set_kernel_flavour(flavour)
            d = c.filter_whole(0, 3, 0, 0).copy(box_lo=lo, box_hi=hi)
            res = c.volume_filter(d, taps)
            assert res.as_tuple() == want_res and c.filter_counters()[0] == want_cnt[0] and c.filter_counters()[2] == 3, flavour
            got = c.volume_download(0, shape)
            assert np.array_equal(vt.bits(got[z0:z1]), vt.bits(want[1:1 + z1 - z0])), flavour
            for sl in (slice(z0 - 8, z0), slice(z1, shape[0]), slice(0, z0 - 8, 16)):
                assert np.array_equal(vt.bits(got[sl]), vt.bits(src[sl])), (flavour, sl)
            del got
            if flavour == 0:
                c.volume_upload(0, src)
    assert want_res[0] == (hi[0] - lo[0]) * (hi[1] - lo[1]) * (z1 - z0) and np.abs(want[1:-1, lo[1]:hi[1], lo[0]:hi[0], 0]).min() > 0.0


def test_everything_derived_is_fresh():
    """After a filter into channel 3 of a rendered slot the next vr_render equals the oracle's frame for the filtered volume, and the
    other tools' reports stay what they were."""
    n = 24
    shape = (n, n, n)
    v = ob.normalize_data(hr.raw_to_vec4(hr.ct_phantom_raw(n)))
    tf = (hr.default_opacity_tf(256), hr.default_color_tf(256))
    step, count = hr.stepping_params(n, n, n)
    u = hr.make_uniforms(W, H, steps_count=count, step_size=step)
    taps = tuple(capi.filter_gaussian(s) for s in (1.5, 1.0, 2.0))
    want, want_res, _ = fr.filter(v, v, 3, 3, taps)
    with capi.Context(W, H, 0) as c:
        c.volume_upload(0, v)
        c.tf_upload(0, *tf)
        c.set_uniforms(vt.to_capi_uniforms(u))
        c.render(capi.BASIC)
        before_frame = c.download()[0]
        seen = (c.morph_counters(), c.dist_counters(), c.resample_counters(), c.mesh_counters(), c.grow_counters(), c.hist_counters())
        assert c.filter_counters() == (0, 0, 0) and c.filter_timing() == (0.0, 0.0, 0.0, 0.0)
        res = c.volume_filter(c.filter_whole(0, 3, 0, 3), taps)
        assert res.as_tuple() == want_res
        timing = c.filter_timing()
        assert all(t >= 0.0 for t in timing) and timing[0] > 0.0 and timing[1] > 0.0 and timing[3] > 0.0
        assert seen == (c.morph_counters(), c.dist_counters(), c.resample_counters(), c.mesh_counters(), c.grow_counters(), c.hist_counters())
        c.render(capi.BASIC)
        frame, _, samples = c.download()
        assert np.array_equal(vt.bits(c.volume_download(0, shape)), vt.bits(want))
    ref, n_ref, _ = ob.render(ob.BASIC, u, [want], [tf], W, H, nthreads=4)
    assert samples == n_ref and n_ref > 0
    assert np.array_equal(vt.bits(frame), vt.bits(ref)) and not np.array_equal(vt.bits(frame), vt.bits(before_frame))


def test_errors_leave_both_slots_untouched(ctx):
    shape = (6, 9, 70)
    nx, ny, nz = rc.n_of(shape)
    src = rc.hostile(shape, 91)
    m = rc.arbitrary_bits(shape, 92)
    ctx.volume_upload(0, src)
    ctx.volume_upload(1, m)
    ctx.volume_upload(2, np.zeros((4, 4, 4, 4), f32))
    w = np.ascontiguousarray(G[2])
    good = ctx.filter_whole(0, 3, 1, 0).copy(radius=(2, 0, 2), taps=(w.ctypes.data, None, w.ctypes.data))
    assert ctx.lib.vr_volume_filter(ctx.h, C.byref(good), C.byref(capi.FilterResult())) == capi.VR_OK
    m = ctx.volume_download(1, shape)
    counters = ctx.filter_counters()
    invalid = [dict(src_slot=-1), dict(src_slot=3), dict(dst_slot=-1), dict(dst_slot=3), dict(src_channel=-1), dict(src_channel=4),
               dict(dst_channel=-1), dict(dst_channel=4), dict(radius=(-1, 0, 2)), dict(radius=(2, 0, 33)), dict(radius=(2, 1, 2)),
               dict(taps=(None, None, w.ctypes.data)), dict(border=-1), dict(border=2), dict(dst_slot=2), dict(box_lo=(-1, 0, 0)),
               dict(box_hi=(nx + 1, ny, nz)), dict(box_hi=(nx, ny, nz + 1)), dict(box_lo=(5, 0, 0), box_hi=(4, ny, nz))]
    for over in invalid:
        d = good.copy(**over)
        assert ctx.lib.vr_volume_filter(ctx.h, C.byref(d), C.byref(capi.FilterResult())) == capi.VR_ERR_INVALID_ARG, over
        assert (ctx.lib.vr_last_error(ctx.h) or b"").decode().startswith("vr_volume_filter"), over
    assert ctx.lib.vr_volume_filter(ctx.h, None, None) == capi.VR_ERR_INVALID_ARG
    assert ctx.lib.vr_volume_filter(None, C.byref(good), None) == capi.VR_ERR_INVALID_ARG
    assert ctx.lib.vr_filter_counters(ctx.h, None) == capi.VR_ERR_INVALID_ARG and ctx.lib.vr_filter_timing(ctx.h, None) == capi.VR_ERR_INVALID_ARG
    for bad in ((3, 3, 1, 0), (-1, 3, 1, 0), (0, 4, 1, 0), (0, -1, 1, 0), (0, 3, 3, 0), (0, 3, -1, 0), (0, 3, 1, 4), (0, 3, 1, -1)):
        assert ctx.lib.vr_filter_whole(ctx.h, *bad, C.byref(capi.FilterDesc())) == capi.VR_ERR_INVALID_ARG, bad
    assert ctx.lib.vr_filter_whole(ctx.h, 0, 3, 1, 0, None) == capi.VR_ERR_INVALID_ARG
    assert ctx.filter_counters() == counters
    assert np.array_equal(vt.bits(ctx.volume_download(1, shape)), vt.bits(m))
    assert np.array_equal(vt.bits(ctx.volume_download(0, shape)), vt.bits(src))
    assert not vt.bits(ctx.volume_download(2, (4, 4, 4))).any()
    assert ctx.lib.vr_volume_filter(ctx.h, C.byref(good), None) == capi.VR_OK  # (a NULL result is fine)
    with capi.Context(W, H, 0) as empty:
        assert empty.filter_counters() == (0, 0, 0) and empty.filter_timing() == (0.0, 0.0, 0.0, 0.0)
        assert empty.lib.vr_volume_filter(empty.h, C.byref(good), None) == capi.VR_ERR_NOT_READY
        err = empty.lib.vr_last_error(empty.h)
        assert err.startswith(b"vr_volume_filter") and b"empty" in err
        assert empty.lib.vr_filter_whole(empty.h, 0, 3, 1, 0, C.byref(capi.FilterDesc())) == capi.VR_ERR_NOT_READY
        with pytest.raises(capi.VrError):  # (the failed call created nothing)
            empty.volume_download(1, shape)


def sweep(n=40, seed=23):
    rng = np.random.default_rng(seed)
    cases = []
    for i in range(n):
        shape = (int(rng.integers(1, 13)), int(rng.integers(1, 21)), int(rng.integers(1, 141)))
        nx, ny, nz = rc.n_of(shape)
        radii = [int(rng.choice([0, 1, 2, 3, 5, 8, 32], p=[0.1, 0.2, 0.2, 0.15, 0.15, 0.15, 0.05])) for _ in range(3)]
        on = [bool(rng.random() < 0.7) for _ in range(3)]
        lo = [int(rng.integers(0, m + 1)) for m in (nx, ny, nz)]
        hi = [int(rng.integers(l, m + 1)) for l, m in zip(lo, (nx, ny, nz))]
        if rng.random() < 0.5:
            lo, hi = [0, 0, 0], [nx, ny, nz]
        in_place = bool(rng.random() < 0.3)
        cases.append(dict(shape=shape, seed=1000 + 2 * i, taps_seed=int(rng.integers(1 << 30)), radii=radii, on=on, lo=tuple(lo), hi=tuple(hi),
                          sc=int(rng.integers(4)), dc=int(rng.integers(4)), border=int(rng.integers(2)),
                          bv=float(rng.choice([0.0, -0.0, 1.5, -2e-41, np.inf])), in_place=in_place, fresh=bool(not in_place and rng.random() < 0.3),
                          hostile=bool(rng.random() < 0.4), flavour=int(rng.integers(2)), layout=int(rng.choice([0, 3]))))
    return cases


SWEEP = sweep()


@pytest.mark.parametrize("i", range(len(SWEEP)))
def test_random_sweep(i):
    case = SWEEP[i]
    shape = case["shape"]
    src = (rc.hostile if case["hostile"] else rc.volume)(shape, case["seed"])
    before = None if case["fresh"] else rc.arbitrary_bits(shape, case["seed"] + 1)
    wr = np.random.default_rng(case["taps_seed"])
    taps = tuple(wr.normal(0.0, 0.4, 2 * r + 1).astype(f32) if on else None for r, on in zip(case["radii"], case["on"]))
    with capi.Context(W, H, 0) as c:
        slots = (0, 0) if case["in_place"] else (0, 2)
        if case["fresh"]:
            c.set_kernel_flavour(case["flavour"])
            c.set_volume_layout(case["layout"])
            c.volume_upload(0, src)
            d = c.filter_whole(0, case["sc"], 2, case["dc"]).copy(border=case["border"], border_value=case["bv"], box_lo=case["lo"], box_hi=case["hi"])
            res = c.volume_filter(d, taps)
            want, want_res, want_cnt = fr.filter(src, None, case["sc"], case["dc"], taps, case["border"], case["bv"], case["lo"], case["hi"])
            computed = np.zeros(src.shape, bool)
            computed[..., case["dc"]] = any(case["on"])
            assert same(c.volume_download(2, shape), want, computed) and res.as_tuple() == want_res and c.filter_counters() == want_cnt, case
        else:
            check(c, src, before, taps, case["sc"], case["dc"], case["border"], case["bv"], (case["lo"], case["hi"]), slots,
                  forms=[(case["flavour"], case["layout"])], what=case)


def test_application_smooth_and_gradient_of_gaussian():
    """Application::Smooth at 1 x 1 x 3 mm equals the restatement fed the same weights (sigma / spacing per axis, truncate 4; z gets no pass
    when its radius is 0); GradientOfGaussian writes channels 0 to 2 and leaves channel 3 alone."""
    from volumerendering_amd import host
    shape = (9, 20, 33)
    vol = rc.volume(shape, 95)
    spacing = (1.0, 1.0, 3.0)
    with host.Application(W, H, 0) as app:
        app.OnStart(capi.BASIC, [host.VolumeFile.from_vec4(vol)])
        c = app.context()
        c.volume_upload(1, vol)
        for sigma_mm in (2.0, 0.3, 0.0):
            taps = tuple(capi.filter_gaussian(sigma_mm / sp) if int(4.0 * sigma_mm / sp + 0.5) > 0 else None for sp in spacing)
            assert [t is None for t in taps] == {2.0: [False] * 3, 0.3: [False, False, True], 0.0: [True] * 3}[sigma_mm]
            res = app.smooth(1, 3, 2, 0, sigma_mm, spacing=spacing)
            before = None if sigma_mm == 2.0 else got
            want, want_res, _ = fr.filter(vol, before, 3, 0, taps)
            got = c.volume_download(2, shape)
            assert np.array_equal(vt.bits(got), vt.bits(want)) and res.as_tuple() == want_res, sigma_mm
        unit = app.smooth(1, 3, 2, 0, 1.0)  # (no spacing: 1 mm)
        want, want_res, _ = fr.filter(vol, got, 3, 0, (capi.filter_gaussian(1.0),) * 3)
        assert np.array_equal(vt.bits(c.volume_download(2, shape)), vt.bits(want)) and unit.as_tuple() == want_res
        app.gradient_of_gaussian(1, 2.0, spacing=spacing)
        g = [[capi.filter_gaussian(2.0 / sp, order) for sp in spacing] for order in (0, 1)]
        want = vol
        for k in range(3):
            want, _, _ = fr.filter(vol, want, 3, k, tuple(g[1 if a == k else 0][a] for a in range(3)))
        got = c.volume_download(1, shape)
        assert np.array_equal(vt.bits(got), vt.bits(want)) and np.array_equal(vt.bits(got[..., 3]), vt.bits(vol[..., 3]))
        assert not np.array_equal(vt.bits(got[..., :3]), vt.bits(vol[..., :3]))
        for bad in (dict(sigma_mm=-1.0), dict(sigma_mm=float("nan")), dict(sigma_mm=2.0, spacing=(1.0, 0.0, 1.0)), dict(sigma_mm=9.0, spacing=(1.0, 1.0, 1.0))):
            with pytest.raises(capi.VrError) as e:
                app.smooth(1, 3, 2, 0, **bad)
            assert e.value.code == capi.VR_ERR_INVALID_ARG, bad
        with pytest.raises(capi.VrError) as e:  # (a derivative needs neighbours: the radius along z comes out 0)
            app.gradient_of_gaussian(1, 0.3, spacing=spacing)
        assert e.value.code == capi.VR_ERR_INVALID_ARG
