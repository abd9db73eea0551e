"""GPU side of the distance maps (vr_mask_distance, csrc/vr_dist.h): the downloaded destination slot EQUAL, bit for bit, to the numpy
restatement (dist_ref.py, pinned on the CPU by tests/test_distance.py), and the result and out[0] equal too -- word and line edges, the
three modes in both kernel forms at unit and anisotropic spacing, every kind of operand with hostile values, the limit and what the
default form leaves uncomputed, the probe, the two laws that tie the distances to vr_mask_morph, squared distances near 2^60, the errors,
the freshness of everything downstream of the channel, a random sweep, and the host surface."""
import ctypes as C

import numpy as np
import pytest

import dist_cases as dc
import dist_ref as dr
import host_ref as hr
import iso_ref as ir
import morph_cases as mc
import oracle_binding as ob
import vrtest as vt
from volumerendering_amd import capi

pytestmark = pytest.mark.gpu
f32 = np.float32
W, H = 64, 48
MODES = [capi.DIST_OUTSIDE, capi.DIST_INSIDE, capi.DIST_SIGNED]
MEDIUM = (21, 37, 70)  # nz, ny, nx: x crosses one word
WIDE = dc.WIDE
FIELDS = {}            # (the crop's set, spacing) -> (D2out, D2in): the restatement's fields are computed once per operand


def desc(shape, mode, box=None, **over):
    """A descriptor from slot 0 contour 0 into slot 1 channel 0: unit spacing, no limit, scale 1, no probe, the whole volume unless a box
    is given."""
    d = capi.DistDesc()
    d.src_slot, d.src_contour, d.dst_slot, d.dst_channel, d.mode, d.probe_slot, d.scale = 0, 0, 1, 0, mode, -1, 1.0
    lo, hi = box if box else dc.whole(shape)
    return d.copy(box_lo=lo, box_hi=hi, **{"spacing": dc.UNIT, **over})


def fields_of(src, d):
    (x0, y0, z0), (x1, y1, z1) = tuple(d.box_lo), tuple(d.box_hi)
    a = dr.member(src[..., d.src_contour])[z0:z1, y0:y1, x0:x1]
    key = (a.shape, a.tobytes(), tuple(d.spacing))
    if key not in FIELDS:
        FIELDS[key] = dr.fields(a, tuple(d.spacing))
    return FIELDS[key]


def check(ctx, d, src, before, probe=None, what=None, d2=None):
    """One vr_mask_distance against the restatement: the destination slot bit for bit, the result, out[0] and out[1] + out[2] == out[0].
    `src`: the source slot's voxels; `before`: the destination slot's before the call (None: an empty slot); `probe`: the probe slot's.
    Returns (result, counters, the downloaded destination)."""
    shape = src.shape[:3]
    res = ctx.mask_distance(d)
    cnt = ctx.dist_counters()
    got = ctx.volume_download(d.dst_slot, shape)
    want, want_res, box = dr.distance(src, before, d.src_contour, d.dst_channel, d.mode, tuple(d.box_lo), tuple(d.box_hi), tuple(d.spacing),
                                      int(d.limit), f32(d.scale), probe, d.probe_contour, d2=d2 or fields_of(src, d))
    bad = np.argwhere(vt.bits(got) != vt.bits(want))
    assert bad.size == 0, (what, len(bad), bad[:4], got[tuple(bad[0][:3])], want[tuple(bad[0][:3])])
    assert res.as_tuple() == want_res, (what, res.as_tuple(), want_res)
    assert cnt[0] == box and cnt[1] + cnt[2] == cnt[0], (what, cnt, box)
    return res, cnt, got


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


@pytest.mark.parametrize("shape", dc.EDGE_SHAPES, ids=["70x9x6", "130x37x21", "64x4x4", "70x1x5", "1x6x9"])
def test_word_and_line_edges(ctx, shape):
    """x crossing one word, three words, exactly one word, rows of one voxel, slices of one row; boxes aligned neither to 4 nor to 64, at
    word borders, empty and of one voxel; the three modes in both kernel forms at unit spacing and at 1 x 1 x 3 mm."""
    src = mc.hostile(dc.dense(shape, seed=21), 0, seed=22)
    state = dc.arbitrary_bits(shape, seed=23)
    ctx.volume_upload(0, src)
    ctx.volume_upload(1, state)
    seen = 0
    for box in dc.boxes(shape):
        for spacing in (dc.UNIT, dc.MM):
            for mode in MODES:
                for flavour in (0, 1):
                    ctx.set_kernel_flavour(flavour)
                    d = desc(shape, mode, box, spacing=spacing, dst_channel=mode + 1)
                    res, cnt, state = check(ctx, d, src, state, what=(box, spacing, mode, flavour))
                    seen = max(seen, res.src_voxels)
                    if flavour == 1:
                        assert cnt[1] == cnt[0]
    assert seen > 16  # (not vacuous)


@pytest.mark.parametrize("name", ["empty", "full", "noise", "dense", "shell"])
def test_operands(ctx, name):
    """Every kind of operand as a mask of hostile values (NaN, -0.0f, denormals), into a destination of arbitrary bits whose other three
    components and whose voxels outside the box keep them; at 1 x 1 x 3 mm in millimetres."""
    shape = MEDIUM
    src = mc.hostile(dc.operands(shape)[name], 3, seed=44)
    state = dc.arbitrary_bits(shape, seed=43)
    ctx.volume_upload(0, src)
    ctx.volume_upload(1, state)
    box = ((3, 2, 1), (67, 35, 20))
    for mode in MODES:
        for flavour in (0, 1):
            ctx.set_kernel_flavour(flavour)
            d = desc(shape, mode, box, src_contour=3, dst_channel=2, spacing=dc.MM, scale=0.001)
            res, cnt, state = check(ctx, d, src, state, what=(name, mode, flavour))
            inside = state[1:20, 2:35, 3:67, 2]
            if name == "empty":  # +inf without a limit, except where the INSIDE field is 0
                assert res.src_voxels == 0 and (np.isposinf(inside).all() if mode != capi.DIST_INSIDE else not inside.any())
                assert res.beyond == (0 if mode == capi.DIST_INSIDE else cnt[0])
            if name == "full":  # (what lies outside the box is neither: B' is empty)
                assert res.src_voxels == cnt[0] == 64 * 33 * 19 and (tuple(res.lo), tuple(res.hi)) == box
                assert np.isneginf(inside).all() if mode == capi.DIST_SIGNED else np.isposinf(inside).all() if mode == capi.DIST_INSIDE else not inside.any()
            if name in ("noise", "dense", "shell"):
                assert res.beyond == 0 and np.isfinite(inside).all()
                if mode == capi.DIST_SIGNED:
                    assert not (inside == 0).any() and np.array_equal(inside < 0, dr.member(src[1:20, 2:35, 3:67, 3]))


def test_single_voxels_and_in_place(ctx):
    """A single voxel at each corner and at x = 63 / 64 of a 130-wide volume; then source and destination the same slot and component."""
    shape = WIDE
    state = np.zeros(shape + (4,), f32)
    ctx.volume_upload(1, state)
    for k, (x, y, z) in enumerate(dc.corners(shape)):
        src = np.zeros(shape + (4,), f32)
        src[z, y, x, 0] = f32(np.nan)
        ctx.volume_upload(0, src)
        ctx.set_kernel_flavour(k % 2)
        d2out = dr.d2_from_points(shape, [(x, y, z)], dc.MM)
        d2in = np.where(dc.points(shape, [(x, y, z)]), np.int64(min(s * s for s, n in zip(dc.MM, shape[::-1]) if n > 1)), np.int64(0))
        for mode in (capi.DIST_OUTSIDE, capi.DIST_SIGNED):
            res, _, state = check(ctx, desc(shape, mode, spacing=dc.MM, scale=0.001), src, state, what=(x, y, z, mode), d2=(d2out, d2in))
            assert res.src_voxels == 1 and tuple(res.lo) == (x, y, z)
    src = mc.hostile(dc.shell(shape), 2, seed=45)
    for mode in MODES:
        for flavour in (0, 1):
            ctx.set_kernel_flavour(flavour)
            ctx.volume_upload(0, src)
            d = desc(shape, mode, ((2, 1, 0), (129, 37, 20)), src_contour=2, dst_slot=0, dst_channel=2)
            check(ctx, d, src, src, what=("in place", mode, flavour))


def test_limit_and_settling(ctx):
    """Four voxels in 130 x 37 x 21 with a small limit: the default form computes a part of the box, flavour 1 all of it, and the slots
    are identical; `beyond` and the saturated value are as defined.  Without a limit an empty A' gives +inf everywhere."""
    shape = WIDE
    small = np.zeros(shape + (4,), f32)
    small[10, 18, 40:44, 0] = 1.0
    ctx.volume_upload(0, small)
    state = dc.arbitrary_bits(shape, seed=73)
    ctx.volume_upload(1, state)
    for mode in MODES:
        ctx.set_kernel_flavour(0)
        d = desc(shape, mode, spacing=dc.MM, limit=5000, scale=0.001, dst_channel=1)
        res0, cnt0, after0 = check(ctx, d, small, state, what=(mode, 0))
        assert 0 < cnt0[1] < cnt0[0] and cnt0[2] > 0
        ctx.set_kernel_flavour(1)
        res1, cnt1, after1 = check(ctx, d, small, after0, what=(mode, 1))
        assert cnt1[1] == cnt1[0] and res1.as_tuple() == res0.as_tuple() and np.array_equal(vt.bits(after0), vt.bits(after1))
        ch = after0[..., 1]
        if mode == capi.DIST_INSIDE:  # (every voxel of A' has a neighbour in B' at 1 mm)
            assert res0.beyond == 0 and float(ch.max()) == float(f32(1000.0) * f32(0.001))
        else:
            ball = int((fields_of(small, d)[0] <= 5000 ** 2).sum())
            assert res0.beyond == cnt0[0] - ball and int((ch == f32(5000.0) * f32(0.001)).sum()) >= res0.beyond > 0
            assert float(ch.max()) == float(f32(5000.0) * f32(0.001))
        state = after1
    ctx.set_kernel_flavour(0)
    ctx.volume_upload(0, np.zeros(shape + (4,), f32))
    res, cnt, after = check(ctx, desc(shape, capi.DIST_OUTSIDE, spacing=dc.MM), np.zeros(shape + (4,), f32), state)
    assert np.isposinf(after[..., 0]).all() and res.beyond == cnt[0] and cnt[1] == 0
    res, cnt, after = check(ctx, desc(shape, capi.DIST_OUTSIDE, spacing=dc.MM, limit=7), np.zeros(shape + (4,), f32), after)
    assert (after[..., 0] == 7.0).all() and res.beyond == cnt[0]


def test_probe(ctx):
    """probe_min_sq / probe_max_sq of D2out over a probe that overlaps the structure, is disjoint from it, is empty, lies beyond the limit;
    the probe may be the destination."""
    shape = MEDIUM
    a = np.zeros(shape, bool)
    a[5:12, 10:20, 20:40] = True
    src = mc.hostile(a, 0, seed=51)
    ctx.volume_upload(0, src)
    p = np.zeros(shape, bool)
    p[8:15, 15:30, 35:60] = True   # contour 0: overlaps A'
    q = np.zeros(shape, bool)
    q[15:20, 25:36, 50:69] = True  # contour 1: disjoint from it
    probe = mc.hostile(p, 0, seed=52)
    probe[..., 1] = mc.hostile(q, 1, seed=53)[..., 1]
    probe[..., 2] = f32(-0.0)      # contour 2: empty
    seen = []
    for mode in (capi.DIST_OUTSIDE, capi.DIST_SIGNED):
        for contour in (0, 1, 2):
            for limit in (0, 9000):
                for flavour in (0, 1):
                    ctx.set_kernel_flavour(flavour)
                    ctx.volume_upload(1, probe)
                    d = desc(shape, mode, ((1, 0, 2), (70, 36, 21)), spacing=dc.MM, limit=limit, probe_slot=1, probe_contour=contour, dst_channel=3)
                    res, _, _ = check(ctx, d, src, probe, probe=probe, what=(mode, contour, limit, flavour))
                    seen.append((contour, limit, res.probe_voxels, res.probe_min_sq, res.probe_max_sq))
                    # the probe's own contour as the destination
                    ctx.volume_upload(1, probe)
                    d = d.copy(dst_channel=contour)
                    check(ctx, d, src, probe, probe=probe, what=("probe is the destination", mode, contour, limit, flavour))
    assert all(n > 0 and lo == 0 and 0 < hi < dr.U64_MAX for c, limit, n, lo, hi in seen if c == 0 and limit == 0)
    assert all(n > 0 and 0 < lo < hi < dr.U64_MAX for c, limit, n, lo, hi in seen if c == 1 and limit == 0)
    assert all((n, lo, hi) == (0, 0, 0) for c, limit, n, lo, hi in seen if c == 2)
    assert all(n > 0 and lo == hi == dr.U64_MAX for c, limit, n, lo, hi in seen if c == 1 and limit == 9000)  # (beyond 9 mm)
    assert all(n > 0 and lo == 0 and hi == dr.U64_MAX for c, limit, n, lo, hi in seen if c == 0 and limit == 9000)


@pytest.mark.parametrize("kind", ["dense", "sparse"])
def test_the_morph_laws_on_the_device(ctx, kind):
    """vr_mask_distance, then a threshold on the download, against vr_mask_morph with vr_morph_ball at 1 x 1 x 3 mm, r = 5 mm:
    { D2out <= r^2 } is DILATE and { p in box : D2in > r^2 } is ERODE.  The threshold on the f32 channel (scale 1) is exact: every D2 is a
    multiple of 10^6 here, r^2 = 25 * 10^6 and its root 5000 are exact in f32, the conversion and the square root are monotone, and the
    next D2, 26 * 10^6, has a root above 5099."""
    shape = MEDIUM
    r = 5000
    a = dc.dense(shape, seed=61) if kind == "dense" else dc.sparse(shape, seed=62)
    src = mc.hostile(a, 1, seed=63)
    box = ((2, 1, 1), (69, 36, 20))
    crop = (slice(1, 20), slice(1, 36), slice(2, 69))
    ctx.volume_upload(0, src)
    ctx.volume_upload(1, np.zeros(shape + (4,), f32))
    element = capi.morph_ball(dc.MM, r)
    for op in (capi.MORPH_DILATE, capi.MORPH_ERODE):
        ctx.mask_morph(capi.MorphDesc().copy(src_slot=0, src_contour=1, dst_slot=1, dst_contour=op, op=op, combine=capi.MORPH_REPLACE,
                                             box_lo=box[0], box_hi=box[1], element=element))
    morphed = ctx.volume_download(1, shape)
    dilated, eroded = (morphed[..., op][crop] == 1.0 for op in (capi.MORPH_DILATE, capi.MORPH_ERODE))
    state = np.zeros(shape + (4,), f32)
    ctx.volume_upload(2, state)
    for flavour in (0, 1):
        ctx.set_kernel_flavour(flavour)
        _, _, state = check(ctx, desc(shape, capi.DIST_OUTSIDE, box, src_contour=1, dst_slot=2, dst_channel=0, spacing=dc.MM), src, state)
        _, _, state = check(ctx, desc(shape, capi.DIST_INSIDE, box, src_contour=1, dst_slot=2, dst_channel=1, spacing=dc.MM), src, state)
        assert np.array_equal(state[..., 0][crop] <= f32(r), dilated), (kind, flavour)
        assert np.array_equal(state[..., 1][crop] > f32(r), eroded), (kind, flavour)
    assert dilated.sum() > a[crop].sum() > eroded.sum()
    if kind == "dense":
        assert eroded.sum() > 0


@pytest.mark.parametrize("axis", [0, 2], ids=["x", "z"])
def test_magnitudes(axis):
    """65535 voxels at spacing 16384: the largest legal extent, (65534 * 16384)^2 = 2^60 - 2^45 + 2^28.  Along x the bit-row pass alone
    meets it (65535 x 1 x 2), along z the envelope pass (2 x 1 x 65535 voxels).  The channel, probe_min_sq and probe_max_sq are exact;
    spacing 16385 is VR_ERR_INVALID_ARG."""
    n = 65535
    shape = (2, 1, n) if axis == 0 else (n, 1, 2)
    spacing = (16384, 7, 1 << 20) if axis == 0 else (1 << 20, 7, 16384)
    at = (lambda i, j: (i, 0, j)) if axis == 0 else (lambda i, j: (j, 0, i))  # (x, y, z) of position i along the long axis, j across
    with capi.Context(W, H, 0) as c:
        for k, (ends, probes) in enumerate((([0], [n - 1, 1]), ([0, n - 1], [n // 2, 5]), ([n - 1], [0]), ([0, 63, 64, 40000], [65000, 64]))):
            pts = [at(i, 0) for i in ends]
            src = np.zeros(shape + (4,), f32)
            probe = np.zeros(shape + (4,), f32)
            for x, y, z in pts:
                src[z, y, x, 0] = 1.0
            for i in probes:
                x, y, z = at(i, 1)
                probe[z, y, x, 0] = 1.0
            c.volume_upload(0, src)
            c.volume_upload(1, probe)
            d2out = dr.d2_from_points(shape, pts, spacing)
            d2in = np.where(d2out == 0, np.int64(min(16384 ** 2, (1 << 20) ** 2)), np.int64(0))  # (the nearest voxel of B' is a neighbour)
            c.set_kernel_flavour(k % 2)
            for mode in (capi.DIST_OUTSIDE, capi.DIST_SIGNED):
                d = desc(shape, mode, spacing=spacing, probe_slot=1, probe_contour=0, dst_slot=2, dst_channel=3, scale=0.001)
                before = None if (k, mode) == (0, capi.DIST_OUTSIDE) else got
                res, cnt, got = check(c, d, src, before, probe=probe, what=(axis, ends, mode), d2=(d2out, d2in))
                want = sorted(int(d2out[z, y, x]) for x, y, z in (at(i, 1) for i in probes))
                assert (res.probe_voxels, res.probe_min_sq, res.probe_max_sq) == (len(probes), want[0], want[-1])
            if ends == [0]:
                assert res.probe_max_sq == (65534 * 16384) ** 2 + (1 << 40) and res.probe_max_sq > 1 << 59
        bad = desc(shape, capi.DIST_OUTSIDE, spacing=tuple(16385 if s == 16384 else s for s in spacing), dst_slot=2, dst_channel=3)
        assert c.lib.vr_mask_distance(c.h, C.byref(bad), None) == capi.VR_ERR_INVALID_ARG
        assert b"2^30" in c.lib.vr_last_error(c.h)
        assert np.array_equal(vt.bits(c.volume_download(2, shape)), vt.bits(got))


def test_errors_leave_the_destination_untouched(ctx):
    shape = (13, 18, 23)
    nz, ny, nx = shape
    src = mc.hostile(dc.dense(shape, seed=81), 0, seed=82)
    m = dc.arbitrary_bits(shape, seed=83)
    ctx.volume_upload(0, src)
    ctx.volume_upload(1, m)
    ctx.volume_upload(2, np.zeros((4, 4, 4, 4), f32))
    good = desc(shape, capi.DIST_SIGNED, spacing=dc.MM, limit=4000, scale=0.001, probe_slot=1, probe_contour=2)
    check(ctx, good, src, m, probe=m)
    m = ctx.volume_download(1, shape)
    counters = ctx.dist_counters()
    invalid = [dict(src_slot=-1), dict(src_slot=3), dict(dst_slot=-1), dict(dst_slot=3), dict(src_contour=-1), dict(src_contour=4),
               dict(dst_channel=-1), dict(dst_channel=4), dict(mode=-1), dict(mode=3), dict(probe_slot=-2), dict(probe_slot=3),
               dict(probe_contour=-1), dict(probe_contour=4), dict(mode=capi.DIST_INSIDE),  # (a probe with INSIDE)
               dict(spacing=(0, 1000, 3000)), dict(spacing=(1000, 0, 3000)), dict(spacing=(1000, 1000, (1 << 20) + 1)),
               dict(limit=(1 << 31) + 1), dict(scale=0.0), dict(scale=-1.0), dict(scale=float("inf")), dict(scale=float("nan")),
               dict(box_lo=(-1, 0, 0)), dict(box_hi=(nx + 1, ny, nz)), dict(box_hi=(nx, ny, nz + 1)), dict(box_lo=(5, 0, 0), box_hi=(4, ny, nz)),
               dict(dst_slot=2), dict(src_slot=2, dst_slot=1), dict(probe_slot=2)]
    # (the rule for the box's extent needs an axis beyond 1024 voxels: test_magnitudes)
    for over in invalid:
        d = good.copy(**over)
        assert ctx.lib.vr_mask_distance(ctx.h, C.byref(d), C.byref(capi.DistResult())) == capi.VR_ERR_INVALID_ARG, over
        assert (ctx.lib.vr_last_error(ctx.h) or b"").decode().startswith("vr_mask_distance"), over
    assert ctx.lib.vr_mask_distance(ctx.h, None, None) == capi.VR_ERR_INVALID_ARG
    assert (ctx.lib.vr_last_error(ctx.h) or b"").decode().startswith("vr_mask_distance")
    assert ctx.lib.vr_mask_distance(None, C.byref(good), None) == capi.VR_ERR_INVALID_ARG
    assert ctx.lib.vr_dist_counters(ctx.h, None) == capi.VR_ERR_INVALID_ARG
    assert ctx.lib.vr_dist_timing(ctx.h, None) == capi.VR_ERR_INVALID_ARG
    assert ctx.dist_counters() == counters
    assert np.array_equal(vt.bits(ctx.volume_download(1, shape)), vt.bits(m))
    assert np.array_equal(vt.bits(ctx.volume_download(0, shape)), vt.bits(src))
    assert np.array_equal(vt.bits(ctx.volume_download(2, (4, 4, 4))), np.zeros((4, 4, 4, 4), np.uint32))
    # the largest legal values pass
    check(ctx, good.copy(limit=1 << 31, spacing=(1 << 20, 1 << 20, 1 << 20)), src, m, probe=m)
    m = ctx.volume_download(1, shape)
    with capi.Context(W, H, 0) as empty:
        assert empty.dist_counters() == (0, 0, 0) and empty.dist_timing() == (0.0, 0.0, 0.0, 0.0)
        assert empty.lib.vr_mask_distance(empty.h, C.byref(good), None) == capi.VR_ERR_NOT_READY
        err = empty.lib.vr_last_error(empty.h)
        assert err.startswith(b"vr_mask_distance") and b"empty" in err
        assert empty.lib.vr_dist_whole(empty.h, 0, 0, 1, 0, capi.DIST_SIGNED, C.byref(capi.DistDesc())) == capi.VR_ERR_NOT_READY
        empty.volume_upload(0, src)  # the probe slot is empty: it is the destination, which the failed call does not create
        assert empty.lib.vr_mask_distance(empty.h, C.byref(good), None) == capi.VR_ERR_NOT_READY
        assert b"probe" in empty.lib.vr_last_error(empty.h)
        with pytest.raises(capi.VrError):
            empty.volume_download(1, shape)
        assert np.array_equal(vt.bits(empty.volume_download(0, shape)), vt.bits(src))
    # vr_dist_whole
    d = ctx.dist_whole(0, 2, 1, 3, capi.DIST_INSIDE)
    assert bytes(d) == bytes(desc(shape, capi.DIST_INSIDE, src_contour=2, dst_channel=3))
    assert bytes(capi.dist_whole(ctx, 0, 2, 1, 3, capi.DIST_INSIDE)) == bytes(d)
    for bad in ((3, 0, 1, 0, 1), (-1, 0, 1, 0, 1), (0, 4, 1, 0, 1), (0, -1, 1, 0, 1), (0, 0, 3, 0, 1), (0, 0, -1, 0, 1), (0, 0, 1, 4, 1),
                (0, 0, 1, -1, 1), (0, 0, 1, 0, 3), (0, 0, 1, 0, -1)):
        assert ctx.lib.vr_dist_whole(ctx.h, *bad, C.byref(capi.DistDesc())) == capi.VR_ERR_INVALID_ARG, bad
    assert ctx.lib.vr_dist_whole(ctx.h, 0, 0, 1, 0, 1, None) == capi.VR_ERR_INVALID_ARG
    # a NULL result is fine
    assert ctx.lib.vr_mask_distance(ctx.h, C.byref(good), None) == capi.VR_OK


def test_everything_downstream_of_the_channel_is_fresh():
    """After a call into channel 3 of slot 0, a histogram of that channel and a slice through it see the new values, and after
    vr_volume_precompute_gradient a VR_VARIANT_ISO frame at level +r equals the frame the restatement pinned to the oracle gives for
    the very volume the slot now holds -- which is the oracle's gradient of the expected channel; what the reporting calls say about
    earlier launches stays."""
    n = 16
    shape = (n, n, n)
    z, y, x = np.meshgrid(*[np.arange(n)] * 3, indexing="ij")
    ball = (x - 7.5) ** 2 + (y - 7.5) ** 2 + (z - 7.5) ** 2 <= 6.2 ** 2
    v = mc.hostile(ball, 3, seed=91)
    v[..., :3] = 0.0
    tf = (np.ones(64, f32), np.tile(np.array([0.8, 0.55, 0.3, 1.0], f32), (64, 1)))
    step, count = hr.stepping_params(n, n, n)
    u = hr.make_uniforms(W, H, steps_count=count, step_size=step)
    level, scale = 0.25, 0.125  # two voxels inside the structure's surface
    with capi.Context(W, H, 0) as ctx:
        ctx.volume_upload(0, v)
        ctx.tf_upload(0, *tf)
        ctx.set_uniforms(vt.to_capi_uniforms(u))
        ctx.set_iso_value(level)
        ctx.render(capi.ISO)
        before_frame = ctx.download()[0]
        hd = ctx.hist_whole(0, 64, 64.0)
        sd = ctx.slice_orthogonal(0, 2, n // 2, 1)
        before_hist, before_img = ctx.histogram(hd), ctx.slice(sd)
        reports = (ctx.counters(), ctx.last_kernel_flavour(), ctx.slice_counters(), ctx.hist_counters(), len(ctx.kernel_times()),
                   ctx.grow_counters(), ctx.morph_counters(), ctx.morph_timing())
        d = ctx.dist_whole(0, 3, 0, 3, capi.DIST_INSIDE).copy(scale=scale)
        res, _, after = check(ctx, d, v, v)
        assert res.src_voxels == int(ball.sum()) and 0.5 < float(after[..., 3].max()) <= 1.0
        assert (ctx.counters(), ctx.last_kernel_flavour(), ctx.slice_counters(), ctx.hist_counters(), len(ctx.kernel_times()),
                ctx.grow_counters(), ctx.morph_counters(), ctx.morph_timing()) == reports
        timing = ctx.dist_timing()
        assert len(timing) == 4 and all(t >= 0.0 for t in timing) and timing[3] > 0.0
        hist, img = ctx.histogram(hd), ctx.slice(sd)
        ctx.volume_precompute_gradient(0)
        lit = ctx.volume_download(0, shape)
        assert np.array_equal(vt.bits(lit), vt.bits(ob.precompute_gradient(after)))
        ctx.render(capi.ISO)
        frame = ctx.download()[0]
        # the same context after an upload of the expected volumes
        ctx.volume_upload(0, after)
        want_hist, want_img = ctx.histogram(hd), ctx.slice(sd)
        ctx.volume_upload(0, lit)
        ctx.render(capi.ISO)
        want_frame = ctx.download()[0]
    assert np.array_equal(hist[0], want_hist[0]) and hist[1] == want_hist[1] and not np.array_equal(hist[0], before_hist[0])
    assert np.array_equal(vt.bits(img), vt.bits(want_img)) and not np.array_equal(vt.bits(img), vt.bits(before_img))
    ref, _, covered = ir.frame(u, W, H, lit, tf, level)
    assert np.array_equal(vt.bits(frame), vt.bits(ref)) and np.array_equal(vt.bits(frame), vt.bits(want_frame))
    assert covered > 0 and not np.array_equal(vt.bits(frame), vt.bits(before_frame))


SWEEP = dc.sweep(40)


@pytest.mark.parametrize("i", range(40))
def test_random_sweep(i):
    case = SWEEP[i]
    shape, seed = case["shape"], case["seed"]
    src = mc.hostile(dc.sweep_set(case), case["src_contour"], seed=seed + 1)
    other = dc.arbitrary_bits(shape, seed=seed + 2)
    vols = {case["src_slot"]: src, 1 - case["src_slot"]: other}  # slots 0 and 1 hold a volume; slot 2 is empty (a fresh destination)
    with capi.Context(W, H, 0) as c:
        c.set_kernel_flavour(i % 2)
        c.set_volume_layout(case["layout"])
        for slot, vol in vols.items():
            c.volume_upload(slot, vol)
        d = capi.DistDesc().copy(src_slot=case["src_slot"], src_contour=case["src_contour"], dst_slot=case["dst_slot"],
                                 dst_channel=case["dst_channel"], mode=case["mode"], probe_slot=-1 if case["probe"] is None else 1,
                                 probe_contour=case["probe"] or 0, limit=case["limit"], spacing=case["spacing"], scale=case["scale"],
                                 box_lo=case["box_lo"], box_hi=case["box_hi"])
        check(c, d, src, vols.get(case["dst_slot"]), probe=None if case["probe"] is None else vols[1], what=case)


def test_application_distance_mm(tmp_path):
    """DistanceMm on a grid of 0.977 x 0.977 x 2.5 mm read from (synthetic) DICOM: micrometre spacings (977, 977, 2500), the limit in
    micrometres, the channel in millimetres."""
    import dicom_writer as dw
    from volumerendering_amd import host, synth
    n, nz = 40, 12
    raw = synth.ct_phantom_raw(n)[:nz]
    folder = tmp_path / "ct"
    folder.mkdir()
    for k in range(nz):
        dw.write_slice(str(folder / f"{k:03d}.dcm"), raw[k], rows=n, cols=n, instance=k + 1, position=(0.0, 0.0, 2.5 * k), spacing=(0.977, 0.977),
                       thickness=2.5, largest=int(raw.max()))
    grid = host.VolumeFile.from_dicom(str(folder))
    shape = (nz, n, n)
    mask = mc.hostile(dc.dense(shape, seed=91), 1, seed=93)
    sp = (977, 977, 2500)
    with host.Application(W, H, 0) as app:
        app.OnStart(capi.BASIC, [grid])
        c = app.context()
        c.volume_upload(1, mask)
        res = app.distance_mm(1, 1, 2, 3, capi.DIST_SIGNED, 7.0, grid)
        got = c.volume_download(2, shape)
        want, want_res, _ = dr.distance(mask, None, 1, 3, dr.SIGNED, *dc.whole(shape), sp, 7000, f32(0.001))
        assert np.array_equal(vt.bits(got), vt.bits(want)) and res.as_tuple() == want_res and res.beyond > 0 and res.src_voxels > 0
        assert float(got[..., 3].max()) == float(f32(7000.0) * f32(0.001))
        res = app.distance_mm(1, 1, 2, 0, capi.DIST_OUTSIDE, 0.0, grid)  # no limit
        want, want_res, _ = dr.distance(mask, got, 1, 0, dr.OUTSIDE, *dc.whole(shape), sp, 0, f32(0.001))
        assert np.array_equal(vt.bits(c.volume_download(2, shape)), vt.bits(want)) and res.as_tuple() == want_res and res.beyond == 0
        # DistanceMap is vr_mask_distance on the application's context
        dsc = c.dist_whole(1, 1, 2, 2, capi.DIST_INSIDE)
        res = app.distance_map(dsc)
        want2, want_res, _ = dr.distance(mask, want, 1, 2, dr.INSIDE, *dc.whole(shape), dc.UNIT)
        assert np.array_equal(vt.bits(c.volume_download(2, shape)), vt.bits(want2)) and res.as_tuple() == want_res
        for bad in (-1.0, float("nan"), float("inf")):
            with pytest.raises(capi.VrError) as e:
                app.distance_mm(1, 1, 2, 0, capi.DIST_SIGNED, bad, grid)
            assert e.value.code == capi.VR_ERR_INVALID_ARG
        with pytest.raises(capi.VrError):  # (not read from DICOM: no spacing)
            app.distance_mm(1, 1, 2, 0, capi.DIST_SIGNED, 7.0, host.VolumeFile.from_raw(raw))
