"""The rank filters on the device (vr_volume_rank, include/vr.h) against the numpy restatement (rank_ref.py): the downloaded destination,
the result struct, all three counters and the untouched source, BIT FOR BIT with no NaN escape -- a rank filter selects and never
computes -- in both kernel forms (flavour 0: LDS tiles; flavour 1: plain) and in the volume layouts 0 and 3.

The default form's tile extents (csrc/vr_rank.h) are the same on all three of its paths (the running minima and maxima of k = 0 and
k = N - 1, the network of the 3 x 3 x 3 median, the radix descent of every other rank): 32 outputs along x, 8 along y, 4 along z.
EDGE_SHAPES holds a volume one below, at and one above each of them, and two tiles plus a tail on two axes at once."""
import ctypes as C

import numpy as np
import pytest

import host_ref as hr
import index_edges_cases as ie
import oracle_binding as ob
import rank_ref as rr
import resample_cases as rc
import vrtest as vt
from volumerendering_amd import capi

pytestmark = pytest.mark.gpu
f32, u32 = np.float32, np.uint32
W, H = 64, 48
FORMS = [(0, 0), (1, 0), (0, 3), (1, 3)]  # (flavour, layout)
SHAPES = [(6, 9, 70), (21, 37, 130), (5, 1, 70), (9, 6, 1)]  # (nz, ny, nx)
EDGE_SHAPES = [(2, 3, 31), (2, 3, 32), (2, 3, 33), (2, 7, 5), (2, 8, 5), (2, 9, 5), (3, 3, 5), (4, 3, 5), (5, 3, 5), (3, 19, 70), (10, 19, 5)]
CLAMP, CONSTANT, MIN, MEDIAN, MAX = capi.FILTER_CLAMP, capi.FILTER_CONSTANT, capi.RANK_MIN, capi.RANK_MEDIAN, capi.RANK_MAX
# NaNs of both signs with distinct payloads (0x7F800001, 0xFFA00000: signalling), +-inf, +-0, denormals, 3e38
HOSTILE_BITS = [0x7FC12345, 0xFFC00001, 0x7F800001, 0xFFA00000, 0x7F800000, 0xFF800000, 0x00000000, 0x80000000, 0x00000001, 0x80000123,
                int(np.array([3e38], f32).view(u32)[0])]


def boxes(shape):
    """The whole volume, a box aligned to nothing, one voxel, an empty box."""
    nx, ny, nz = rc.n_of(shape)
    mid = ((nx // 3, ny // 3, nz // 3), (max(nx // 3 + 1, nx - nx // 4), max(ny // 3 + 1, ny - ny // 5), max(nz // 3 + 1, nz - nz // 3)))
    one = (nx // 2, ny // 2, nz // 2)
    return [((0, 0, 0), (nx, ny, nz)), mid, (one, tuple(v + 1 for v in one)), ((nx // 2, 0, 0), (nx // 2, ny, nz))]


def ranks(radii):
    """{0, 1, N / 2 - 1, N / 2, N / 2 + 1, N - 2, N - 1} and both sentinels."""
    n = rr.window(radii)
    return sorted({k for k in (0, 1, n // 2 - 1, n // 2, n // 2 + 1, n - 2, n - 1) if 0 <= k < n}) + [MEDIAN, MAX]


def describe(ctx, slots, sc, dc, radii, rank, border, border_bits, lo, hi):
    d = ctx.rank_whole(slots[0], sc, slots[1], dc).copy(radius=radii, rank=rank, border=border, box_lo=lo, box_hi=hi)
    # (the bits themselves: a signalling NaN does not survive a conversion to double and back)
    C.c_uint32.from_address(C.addressof(d) + capi.RankDesc.border_value.offset).value = border_bits
    return d


def check(ctx, src, before, radii, rank=MEDIAN, sc=3, dc=0, border=CLAMP, bv=0, box=None, slots=(0, 1), forms=FORMS, what=None):
    """One descriptor in every form against the restatement.  src: the source slot's voxels; before: the destination's before the call
    (ignored in place: slots[0] == slots[1]); bv: the BITS of border_value.  Both slots are uploaded again for every form.  Returns the
    restatement's (volume, result, counters)."""
    shape = src.shape[:3]
    lo, hi = box if box else ((0, 0, 0), rc.n_of(shape))
    in_place = slots[0] == slots[1]
    want, want_res, want_cnt = rr.rank(src, src if in_place else before, sc, dc, radii, rank, border, bv, lo, hi)
    for flavour, layout in forms:
        ctx.set_kernel_flavour(flavour)
        ctx.set_volume_layout(layout)
        ctx.volume_upload(slots[0], src)
        if not in_place:
            ctx.volume_upload(slots[1], before)
        res = ctx.volume_rank(describe(ctx, slots, sc, dc, radii, rank, border, bv, lo, hi))
        cnt = ctx.rank_counters()
        got = ctx.volume_download(slots[1], shape)
        if not np.array_equal(vt.bits(got), vt.bits(want)):
            bad = np.argwhere(vt.bits(got) != vt.bits(want))
            raise AssertionError((what, flavour, layout, len(bad), bad[:4], hex(vt.bits(got)[tuple(bad[0])]), hex(vt.bits(want)[tuple(bad[0])])))
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
    """Volumes with tails on every axis, a single row and a single column; the whole volume, a box aligned to nothing, one voxel and an
    empty box; both borders with a nonzero border value; into a destination of arbitrary bits, whose other components and outside voxels
    keep theirs.  The 3 x 3 x 3 median, a generic rank of an uneven window, and its minimum and maximum."""
    src = rc.volume(shape, 11)
    before = rc.arbitrary_bits(shape, 12)
    for k, box in enumerate(boxes(shape)):
        border, bv = ((CLAMP, 0), (CONSTANT, rr.bits_of(-1.75)))[k % 2]
        _, res, cnt = check(ctx, src, before, (1, 1, 1), MEDIAN, 3, k % 4, border, bv, box, what=(shape, box, "median"))
        assert cnt[2] == (13 if res[0] else 0)
        check(ctx, src, before, (2, 1, 3), 35, 3, (k + 1) % 4, 1 - border, rr.bits_of(0.25), box, what=(shape, box, "generic"))
        check(ctx, src, before, (2, 1, 3), (MIN, MAX)[k % 2], 2, 3, border, bv, box, forms=FORMS[:2], what=(shape, box, "min / max"))


@pytest.mark.parametrize("shape", EDGE_SHAPES, ids=lambda s: "x".join(str(v) for v in s[::-1]))
def test_tile_edges(ctx, shape):
    """One below, at and one above the tile's 32 outputs along x, 8 along y and 4 along z; two tiles and a tail along x and y, and along
    y and z, at once.  Radius 1 and radius 3 on every axis; all three paths of the default form: k = 0 and k = N - 1, the median (the
    network at radius 1, the descent at radius 3) and a generic rank; the whole volume and a box across the tile edges."""
    src = rc.volume(shape, 21)
    before = rc.arbitrary_bits(shape, 22)
    nx, ny, nz = rc.n_of(shape)
    edge = (tuple(max(0, min(n - 2, t - 2)) for n, t in zip((nx, ny, nz), (32, 8, 4))), tuple(min(n, t + 3) for n, t in zip((nx, ny, nz), (32, 8, 4))))
    for r in (1, 3):
        n = (2 * r + 1) ** 3
        for rank in (MIN, MEDIAN, n // 3, MAX):
            check(ctx, src, before, (r, r, r), rank, what=(shape, r, rank))
            check(ctx, src, before, (r, r, r), rank, 1, 2, CONSTANT, rr.bits_of(0.5), edge, forms=FORMS[:2], what=(shape, r, rank, edge))


SMALL = (5, 7, 66)


@pytest.mark.parametrize("radii", [(1, 1, 1), (2, 2, 2), (3, 3, 3), (3, 0, 1), (0, 2, 0)], ids=lambda r: "r" + "-".join(str(v) for v in r))
def test_every_rank(ctx, radii):
    """Every k of the 3 x 3 x 3 window; for the other windows 0, 1, the ranks around the median, N - 2, N - 1 and both sentinels."""
    src = rc.volume(SMALL, 31)
    before = rc.arbitrary_bits(SMALL, 32)
    for rank in (list(range(27)) + [MEDIAN, MAX]) if radii == (1, 1, 1) else ranks(radii):
        border, bv = (CLAMP, 0) if rank % 2 == 0 else (CONSTANT, rr.bits_of(0.125))
        _, _, cnt = check(ctx, src, before, radii, rank, 3, 1, border, bv, what=(radii, rank))
        assert cnt[2] == rr.resolve(rank, radii)


ALL_RADII = [(x, y, z) for x in (0, 1, 3) for y in (0, 1, 3) for z in (0, 1, 3)] + [(2, 2, 1)]


@pytest.mark.parametrize("radii", ALL_RADII, ids=lambda r: "r" + "-".join(str(v) for v in r))
def test_radii(ctx, radii):
    """Every combination of the radii 0, 1 and 3, and (2, 2, 1), at the median, both borders with a border value that is not 0; radius
    (0, 0, 0) is a pure copy that changes nothing."""
    src = rc.hostile(SMALL, 41)
    before = rc.arbitrary_bits(SMALL, 42)
    want, res, _ = check(ctx, src, before, radii, MEDIAN, 3, 0, CLAMP, 0, None, what=radii)
    check(ctx, src, before, radii, MEDIAN, 2, 3, CONSTANT, rr.bits_of(-3.25), boxes(SMALL)[1], forms=FORMS[:2], what=(radii, "constant"))
    if radii == (0, 0, 0):
        assert res[2] == 0 and np.array_equal(vt.bits(want[..., 0]), vt.bits(src[..., 3]))


def test_a_window_larger_than_the_volume(ctx):
    """n = 3 with r = 3 on every axis: 316 of the 343 values of every window are the border's."""
    shape = (3, 3, 3)
    src = rc.volume(shape, 43)
    for border, bv in ((CLAMP, 0), (CONSTANT, rr.bits_of(0.1))):
        for rank in (MIN, 5, 150, MEDIAN, 330, MAX):
            check(ctx, src, rc.arbitrary_bits(shape, 44), (3, 3, 3), rank, 3, 3, border, bv, what=(border, rank))


@pytest.mark.parametrize("kind", ["constant", "two values", "four levels"])
def test_ties(ctx, kind):
    """What a counting selection gets wrong: a constant volume, a volume of two values, data quantised to four levels; radii 1 and 2."""
    shape = (6, 9, 70)
    rng = np.random.default_rng(45)
    if kind == "constant":
        a = np.full(shape, 2.5, f32)
    elif kind == "two values":
        a = np.where(rng.random(shape) < 0.5, f32(-1.0), f32(4.0)).astype(f32)
    else:
        a = (np.floor(rng.random(shape) * 4.0) * 0.5 - 0.75).astype(f32)
    src = rc.volume(shape, 46)
    src[..., 3] = a
    before = rc.arbitrary_bits(shape, 47)
    for radii in ((1, 1, 1), (2, 2, 2)):
        for rank in ranks(radii):
            check(ctx, src, before, radii, rank, 3, 2, CONSTANT, rr.bits_of(4.0), forms=FORMS[:2], what=(kind, radii, rank))
        check(ctx, src, before, radii, MEDIAN, forms=FORMS[2:], what=(kind, radii, "layout 3"))


@pytest.mark.parametrize("shape", [(6, 9, 70), (9, 6, 1)], ids=["70x9x6", "1x6x9"])
def test_hostile_values(ctx, shape):
    """NaNs of both signs with distinct payloads (signalling ones included), +-inf, +-0, denormals and 3e38 in the source and as the border
    value: the total order of the header, every pattern stored with its bits."""
    src = rc.hostile(shape, 51)
    flat = src.view(u32)[..., 3].reshape(-1)
    at = np.random.default_rng(52).choice(flat.size, flat.size // 3, replace=False)
    flat[at] = np.array(HOSTILE_BITS, u32)[np.arange(at.size) % len(HOSTILE_BITS)]
    before = rc.arbitrary_bits(shape, 53)
    for i, bv in enumerate(HOSTILE_BITS):
        radii, rank = [((1, 1, 1), MEDIAN), ((1, 1, 1), MIN), ((2, 1, 1), 17), ((1, 1, 1), MAX)][i % 4]
        want, _, _ = check(ctx, src, before, radii, rank, 3, 2, CONSTANT, bv, forms=FORMS[:2], what=(hex(bv), radii, rank))
        assert set(np.unique(vt.bits(want[..., 2]))) <= set(np.unique(vt.bits(src[..., 3]))) | {bv}
    check(ctx, src, before, (1, 1, 1), MEDIAN, what="clamp")
    check(ctx, src, before, (3, 2, 1), 40, what="clamp, generic")
    zeros = np.where(np.random.default_rng(54).random(shape + (4,)) < 0.5, f32(0.0), f32(-0.0)).astype(f32)
    _, res, _ = check(ctx, zeros, before, (1, 1, 1), MEDIAN, what="signed zeros")
    assert res[3:] == (0x80000000, 0)  # (-0.0f is the least value, +0.0f the greatest)
    nans = np.full(shape + (4,), np.nan, f32)
    nans.view(u32)[..., 3] += np.arange(nans[..., 3].size, dtype=u32).reshape(shape)  # (distinct payloads)
    for rank in (MIN, MEDIAN, 5, MAX):
        _, res, _ = check(ctx, nans, before, (1, 1, 1), rank, forms=FORMS[:2], what=("all nan", rank))
        assert res[:2] == (nans[..., 3].size, nans[..., 3].size) and res[3:] == (0, 0)
    _, res, _ = check(ctx, src, before, (0, 0, 0), MEDIAN, what="copy")
    assert res[2] == 0


def test_in_place_and_a_fresh_destination(ctx):
    """Same slot and same channel; same slot, channel 3 into channel 0; an empty destination slot is created with the source's dimensions
    and zeros, by a whole box, a partial box and an empty box."""
    shape = (21, 37, 130)
    src = rc.volume(shape, 61)
    for radii, rank in (((1, 1, 1), MEDIAN), ((2, 1, 2), MIN), ((1, 2, 1), 20)):
        check(ctx, src, None, radii, rank, 3, 3, slots=(0, 0), what=("same channel", radii))
        check(ctx, src, None, radii, rank, 3, 3, CONSTANT, rr.bits_of(1.0), boxes(shape)[1], slots=(1, 1), forms=FORMS[:2], what=("same channel, box", radii))
        check(ctx, src, None, radii, rank, 3, 0, slots=(0, 0), forms=FORMS[:2], what=("3 -> 0", radii))
    check(ctx, src, None, (0, 0, 0), MEDIAN, 2, 1, slots=(0, 0), forms=FORMS[:2], what="copy in place")
    for box in boxes(shape)[:2] + boxes(shape)[3:]:
        for flavour in (0, 1):
            with capi.Context(W, H, 0) as c:
                c.set_kernel_flavour(flavour)
                c.volume_upload(0, src)
                res = c.volume_rank(describe(c, (0, 2), 3, 1, (1, 1, 1), MEDIAN, CLAMP, 0, box[0], box[1]))
                want, want_res, want_cnt = rr.rank(src, None, 3, 1, (1, 1, 1), MEDIAN, lo=box[0], hi=box[1])
                got = c.volume_download(2, shape)
                assert np.array_equal(vt.bits(got), vt.bits(want)) and res.as_tuple() == want_res and c.rank_counters() == want_cnt
                assert not vt.bits(got[..., [0, 2, 3]]).any()


def test_the_launch_loops_go_round(ctx):
    """33 x 177 x 177 voxels: 2 x 23 x 45 = 2070 tiles for the 2048 workgroups the default form launches at the most, 1 033 857 voxels for
    the 524 288 lanes of the plain form.  The median and k = 0 at radius 1."""
    shape = (177, 177, 33)
    assert 2 * 23 * 45 > 2048 and shape[0] * shape[1] * shape[2] > 524288
    src = np.zeros(shape + (4,), f32)
    src[..., 3] = np.random.default_rng(65).normal(0.0, 1.0, shape).astype(f32)
    before = np.zeros(shape + (4,), f32)
    for rank in (MEDIAN, MIN):
        _, res, cnt = check(ctx, src, before, (1, 1, 1), rank, forms=FORMS[:2], what=rank)
        assert res[0] == cnt[1] == src[..., 3].size and res[2] > 0


@pytest.mark.parametrize("n", ie.RODS, ids=lambda n: "x".join(str(v) for v in n))
def test_rods(ctx, n):
    """Axes of 65535 voxels at radius 1: 2048 tiles along x, 8192 along y, 16384 along z."""
    shape = (n[2], n[1], n[0])
    src = rc.volume(shape, 71)
    before = rc.arbitrary_bits(shape, 72)
    check(ctx, src, before, (1, 1, 1), MEDIAN, forms=FORMS[:3], what=n)
    far = tuple(max(0, v - 70) for v in n)
    check(ctx, src, before, (1, 1, 1), MAX, 3, 1, CONSTANT, rr.bits_of(4.0), (far, n), forms=FORMS[:2], what=(n, "far end"))
    check(ctx, src, before, (1, 1, 1), 9, 3, 1, CONSTANT, rr.bits_of(-4.0), (far, n), forms=FORMS[:2], what=(n, "far end, generic"))


def test_a_slot_of_four_gib():
    """A slot of 512 x 512 x 1032 voxels, 4.03 GiB, median-filtered in place from channel 3 into channel 0 at radius 1, in a box of five
    slabs across voxel index 2^28 (the start of slab z = 1024): the box against the restatement of the slabs around it, and every slab
    near the box and every 16th slab of the rest against the source."""
    shape = (ie.A1[2], ie.A1[1], ie.A1[0])
    z0, z1 = ie.LINE_Z - 2, ie.LINE_Z + 3
    lo, hi = (100, 200, z0), (391, 263, z1)
    src = np.zeros(shape + (4,), f32)
    src[z0 - 4:z1 + 4] = rc.volume((z1 - z0 + 8, shape[1], shape[2]), 81)
    sub = src[z0 - 1:z1 + 1]  # (the windows of the box reach one slab beyond it: no voxel of it reads across a z face of the sub-volume)
    want, want_res, want_cnt = rr.rank(sub, sub, 3, 0, (1, 1, 1), MEDIAN, lo=(lo[0], lo[1], 1), hi=(hi[0], hi[1], 1 + z1 - z0))
    with capi.Context(W, H, 0) as c:
        c.volume_upload(0, src)
        for flavour in (0, 1):
            c.set_kernel_flavour(flavour)
            res = c.volume_rank(describe(c, (0, 0), 3, 0, (1, 1, 1), MEDIAN, CLAMP, 0, lo, hi))
            assert res.as_tuple() == want_res and c.rank_counters() == want_cnt, flavour
            got = c.volume_download(0, shape)
            assert np.array_equal(vt.bits(got[z0:z1]), vt.bits(want[1:1 + z1 - z0])), flavour
            for sl in (slice(z0 - 8, z0), slice(z1, shape[0]), slice(0, z0 - 8, 16)):
                assert np.array_equal(vt.bits(got[sl]), vt.bits(src[sl])), (flavour, sl)
            del got
            if flavour == 0:
                c.volume_upload(0, src)
    assert want_res[0] == (hi[0] - lo[0]) * (hi[1] - lo[1]) * (z1 - z0) > want_res[2] > 0 and want_cnt[2] == 13


def test_everything_derived_is_fresh():
    """After a median into channel 3 of a rendered slot the next vr_render equals the oracle's frame for the filtered volume and differs
    from the frame before, and the other tools' reports stay what they were."""
    n = 24
    shape = (n, n, n)
    v = ob.normalize_data(hr.raw_to_vec4(hr.ct_phantom_raw(n)))
    tf = (hr.default_opacity_tf(256), hr.default_color_tf(256))
    step, count = hr.stepping_params(n, n, n)
    u = hr.make_uniforms(W, H, steps_count=count, step_size=step)
    want, want_res, _ = rr.rank(v, v, 3, 3, (2, 2, 2), MEDIAN)
    with capi.Context(W, H, 0) as c:
        c.volume_upload(0, v)
        c.tf_upload(0, *tf)
        c.set_uniforms(vt.to_capi_uniforms(u))
        c.render(capi.BASIC)
        before_frame = c.download()[0]
        seen = (c.morph_counters(), c.dist_counters(), c.resample_counters(), c.mesh_counters(), c.grow_counters(), c.hist_counters(),
                c.filter_counters())
        assert c.rank_counters() == (0, 0, 0) and c.rank_timing() == (0.0, 0.0, 0.0, 0.0)
        res = c.volume_rank(c.rank_whole(0, 3, 0, 3).copy(radius=(2, 2, 2)))
        assert res.as_tuple() == want_res and res.changed > 0
        timing = c.rank_timing()
        assert all(t >= 0.0 for t in timing) and timing[0] > 0.0 and timing[1] == 0.0 and timing[3] > 0.0
        assert seen == (c.morph_counters(), c.dist_counters(), c.resample_counters(), c.mesh_counters(), c.grow_counters(), c.hist_counters(),
                        c.filter_counters())
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
    good = ctx.rank_whole(0, 3, 1, 0).copy(radius=(2, 0, 1))
    assert (list(good.radius), good.rank, good.border, good.border_value, list(good.box_lo), list(good.box_hi)) == ([2, 0, 1], MEDIAN, CLAMP, 0.0, [0, 0, 0], [nx, ny, nz])
    assert ctx.lib.vr_volume_rank(ctx.h, C.byref(good), C.byref(capi.RankResult())) == capi.VR_OK
    m = ctx.volume_download(1, shape)
    counters = ctx.rank_counters()
    assert counters == (nx * ny * nz, nx * ny * nz, 7)
    invalid = [dict(src_slot=-1), dict(src_slot=3), dict(dst_slot=-1), dict(dst_slot=3), dict(src_channel=-1), dict(src_channel=4),
               dict(dst_channel=-1), dict(dst_channel=4), dict(radius=(-1, 0, 2)), dict(radius=(2, 0, 4)), dict(radius=(2, 33, 1)),
               dict(rank=15), dict(rank=-3), dict(rank=1 << 30), dict(radius=(0, 0, 0), rank=1), dict(border=-1), dict(border=2), dict(dst_slot=2),
               dict(box_lo=(-1, 0, 0)), dict(box_hi=(nx + 1, ny, nz)), dict(box_hi=(nx, ny, nz + 1)), dict(box_lo=(5, 0, 0), box_hi=(4, ny, nz))]
    for over in invalid:
        d = good.copy(**over)
        assert ctx.lib.vr_volume_rank(ctx.h, C.byref(d), C.byref(capi.RankResult())) == capi.VR_ERR_INVALID_ARG, over
        assert (ctx.lib.vr_last_error(ctx.h) or b"").decode().startswith("vr_volume_rank"), over
    assert ctx.lib.vr_volume_rank(ctx.h, None, None) == capi.VR_ERR_INVALID_ARG
    assert ctx.lib.vr_volume_rank(None, C.byref(good), None) == capi.VR_ERR_INVALID_ARG
    assert ctx.lib.vr_rank_counters(ctx.h, None) == capi.VR_ERR_INVALID_ARG and ctx.lib.vr_rank_timing(ctx.h, None) == capi.VR_ERR_INVALID_ARG
    for bad in ((3, 3, 1, 0), (-1, 3, 1, 0), (0, 4, 1, 0), (0, -1, 1, 0), (0, 3, 3, 0), (0, 3, -1, 0), (0, 3, 1, 4), (0, 3, 1, -1)):
        assert ctx.lib.vr_rank_whole(ctx.h, *bad, C.byref(capi.RankDesc())) == capi.VR_ERR_INVALID_ARG, bad
    assert ctx.lib.vr_rank_whole(ctx.h, 0, 3, 1, 0, None) == capi.VR_ERR_INVALID_ARG
    assert ctx.rank_counters() == counters
    assert np.array_equal(vt.bits(ctx.volume_download(1, shape)), vt.bits(m))
    assert np.array_equal(vt.bits(ctx.volume_download(0, shape)), vt.bits(src))
    assert not vt.bits(ctx.volume_download(2, (4, 4, 4))).any()
    assert ctx.lib.vr_volume_rank(ctx.h, C.byref(good.copy(rank=14)), None) == capi.VR_OK  # (a NULL result is fine; 14 = N - 1 is a rank)
    assert ctx.rank_counters() == (nx * ny * nz, nx * ny * nz, 14)
    with capi.Context(W, H, 0) as empty:
        assert empty.rank_counters() == (0, 0, 0) and empty.rank_timing() == (0.0, 0.0, 0.0, 0.0)
        assert empty.lib.vr_volume_rank(empty.h, C.byref(good), None) == capi.VR_ERR_NOT_READY
        err = empty.lib.vr_last_error(empty.h)
        assert err.startswith(b"vr_volume_rank") and b"empty" in err
        assert empty.lib.vr_rank_whole(empty.h, 0, 3, 1, 0, C.byref(capi.RankDesc())) == capi.VR_ERR_NOT_READY
        assert empty.rank_counters() == (0, 0, 0) and empty.rank_timing() == (0.0, 0.0, 0.0, 0.0)
        with pytest.raises(capi.VrError):  # (the failed call created nothing)
            empty.volume_download(1, shape)


def sweep(n=40, seed=29):
    rng = np.random.default_rng(seed)
    cases = []
    for i in range(n):
        shape = (int(rng.integers(1, 13)), int(rng.integers(1, 21)), int(rng.integers(1, 141)))
        nx, ny, nz = rc.n_of(shape)
        radii = tuple(int(rng.choice([0, 1, 2, 3], p=[0.2, 0.4, 0.2, 0.2])) for _ in range(3))
        nwin = rr.window(radii)
        rank = [MEDIAN, MIN, MAX, int(rng.integers(0, nwin)), int(rng.integers(0, nwin))][int(rng.integers(5))]
        lo = [int(rng.integers(0, m + 1)) for m in (nx, ny, nz)]
        hi = [int(rng.integers(l, m + 1)) for l, m in zip(lo, (nx, ny, nz))]
        if rng.random() < 0.5:
            lo, hi = [0, 0, 0], [nx, ny, nz]
        in_place = bool(rng.random() < 0.3)
        cases.append(dict(shape=shape, seed=2000 + 2 * i, radii=radii, rank=rank, lo=tuple(lo), hi=tuple(hi), sc=int(rng.integers(4)),
                          dc=int(rng.integers(4)), border=int(rng.integers(2)),
                          bv=int(rng.choice(HOSTILE_BITS + [rr.bits_of(1.5), rr.bits_of(-0.25)])), in_place=in_place,
                          fresh=bool(not in_place and rng.random() < 0.3), data=("hostile", "quantised", "plain")[int(rng.integers(3))],
                          flavour=int(rng.integers(2)), layout=int(rng.choice([0, 3]))))
    return cases


SWEEP = sweep()


@pytest.mark.parametrize("i", range(len(SWEEP)))
def test_random_sweep(i):
    case = SWEEP[i]
    shape = case["shape"]
    if case["data"] == "hostile":
        src = rc.hostile(shape, case["seed"])
    elif case["data"] == "quantised":
        src = (np.floor(rc.volume(shape, case["seed"]) * 2.0) * 0.5).astype(f32)  # (heavy ties)
    else:
        src = rc.volume(shape, case["seed"])
    before = None if case["fresh"] else rc.arbitrary_bits(shape, case["seed"] + 1)
    args = (case["radii"], case["rank"], case["sc"], case["dc"], case["border"], case["bv"])
    with capi.Context(W, H, 0) as c:
        if case["fresh"]:
            c.set_kernel_flavour(case["flavour"])
            c.set_volume_layout(case["layout"])
            c.volume_upload(0, src)
            res = c.volume_rank(describe(c, (0, 2), case["sc"], case["dc"], case["radii"], case["rank"], case["border"], case["bv"], case["lo"], case["hi"]))
            want, want_res, want_cnt = rr.rank(src, None, case["sc"], case["dc"], case["radii"], case["rank"], case["border"], case["bv"], case["lo"], case["hi"])
            assert np.array_equal(vt.bits(c.volume_download(2, shape)), vt.bits(want)) and res.as_tuple() == want_res and c.rank_counters() == want_cnt, case
        else:
            check(c, src, before, *args, (case["lo"], case["hi"]), (0, 0) if case["in_place"] else (0, 2), forms=[(case["flavour"], case["layout"])], what=case)


def test_application_median_and_rank_filter():
    """Application::Median and RankFilter at 1 x 1 x 3 mm equal the restatement with the radii (int)(radius_mm / spacing + 0.5) per axis;
    an over-large radius and a bad spacing are VR_ERR_INVALID_ARG."""
    from volumerendering_amd import host
    shape = (9, 20, 33)
    vol = rc.volume(shape, 95)
    spacing = (1.0, 1.0, 3.0)
    with host.Application(W, H, 0) as app:
        app.OnStart(capi.BASIC, [host.VolumeFile.from_vec4(vol)])
        c = app.context()
        c.volume_upload(1, vol)
        got = None
        for radius_mm, radii in ((2.0, (2, 2, 1)), (1.0, (1, 1, 0)), (1.5, (2, 2, 1)), (0.4, (0, 0, 0)), (3.0, (3, 3, 1))):
            assert radii == tuple(int(radius_mm / sp + 0.5) for sp in spacing)
            res = app.median(1, 3, 2, 0, radius_mm, spacing=spacing)
            want, want_res, want_cnt = rr.rank(vol, got, 3, 0, radii, MEDIAN)
            got = c.volume_download(2, shape)
            assert np.array_equal(vt.bits(got), vt.bits(want)) and res.as_tuple() == want_res and c.rank_counters() == want_cnt, radius_mm
        for rank in (MIN, MAX, 7):
            res = app.rank_filter(1, 3, 2, 1, 2.0, rank, spacing=spacing)
            want, want_res, _ = rr.rank(vol, got, 3, 1, (2, 2, 1), rank)
            got = c.volume_download(2, shape)
            assert np.array_equal(vt.bits(got), vt.bits(want)) and res.as_tuple() == want_res, rank
        unit = app.median(1, 3, 2, 0, 1.0)  # (no spacing: 1 mm)
        want, want_res, _ = rr.rank(vol, got, 3, 0, (1, 1, 1), MEDIAN)
        assert np.array_equal(vt.bits(c.volume_download(2, shape)), vt.bits(want)) and unit.as_tuple() == want_res
        for bad in (dict(radius_mm=-1.0), dict(radius_mm=float("nan")), dict(radius_mm=float("inf")), dict(radius_mm=2.0, spacing=(1.0, 0.0, 1.0)),
                    dict(radius_mm=2.0, spacing=(1.0, float("nan"), 1.0)), dict(radius_mm=3.5, spacing=(1.0, 1.0, 1.0)), dict(radius_mm=2.0, spacing=(0.5, 1.0, 1.0))):
            with pytest.raises(capi.VrError) as e:
                app.median(1, 3, 2, 0, **bad)
            assert e.value.code == capi.VR_ERR_INVALID_ARG, bad
        with pytest.raises(capi.VrError) as e:  # (343 is no rank of a window of 5 x 5 x 3)
            app.rank_filter(1, 3, 2, 0, 2.0, 343, spacing=spacing)
        assert e.value.code == capi.VR_ERR_INVALID_ARG
