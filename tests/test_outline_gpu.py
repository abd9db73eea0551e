"""GPU side of contour tracing (vr_mask_outlines, csrc/vr_outline.h): points, polygons, result and the first two counters EQUAL to the
numpy restatement (outline_ref.py, pinned on the CPU by tests/test_outline.py) -- word and box edges on arbitrary bits, saddles under
both rules, loops of thousands of corners in both kernel forms, 65535-voxel axes and the ends of the coordinate range, the round trip
through vr_mask_polygons on the device, a trace behind a grow and a dilation, no side effects, the capacities, the errors, a random
sweep, and the host surface."""
import ctypes as C

import numpy as np
import pytest

import host_ref as hr
import morph_cases as mc
import outline_cases as oc
import outline_ref as orf
import vrtest as vt
from volumerendering_amd import capi

pytestmark = pytest.mark.gpu
f32 = np.float32
W, H = 64, 48
CT = oc.GRIDS[1]  # 977 x 977 off a negative origin
EMPTY = (0, 0, (0,) * 4, (0,) * 4, (0,) * 4)


def desc(shape, grid=oc.GRIDS[0], box=None, offset=(0, 0), **over):
    """A descriptor on slot 0: contour 0, SPLIT, the whole volume unless a box is given."""
    d = capi.OutlinesDesc()
    d.src_slot, d.contours, d.connect = 0, 1, capi.OUTLINE_SPLIT
    lo, hi = box if box else mc.whole(shape)
    return d.copy(box_lo=lo, box_hi=hi, spacing=grid[0], origin=grid[1], offset=offset, **over)


def reference(d, m, plain=False):
    return orf.trace(m, d.contours, d.connect, tuple(d.box_lo), tuple(d.box_hi), tuple(d.origin), tuple(d.spacing), tuple(d.offset), plain)


def check(ctx, d, m, plain=False, what=None, want=None):
    """One vr_mask_outlines against the restatement: points, polygons, result, out[0:2].  m: the members (4, nz, ny, nx) of the source
    slot; want: the restatement of this very call where a test has it already (everything but its rounds is the same in both kernel
    forms).  Returns (points, polygons, result, counters, the restatement's dict)."""
    pts, polys, res = ctx.mask_outlines(d)
    cnt = ctx.outlines_counters()
    want = want or reference(d, m, plain)
    assert res.as_tuple() == want["result"], (what, res.as_tuple(), want["result"])
    assert polys == want["polygons"], (what, [(a, b) for a, b in zip(polys, want["polygons"]) if a != b][:4])
    bad = np.argwhere(pts != want["points"])
    assert pts.shape == want["points"].shape and bad.size == 0, (what, len(bad), bad[:4])
    assert cnt[:2] == want["result"][:2], (what, cnt, want["result"][:2])
    return pts, polys, res, cnt, want


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


@pytest.mark.parametrize("shape", oc.WORD_EDGE_SHAPES, ids=["70x9x6", "130x37x21", "64x4x4", "65x5x3"])
def test_word_and_box_edges(ctx, shape):
    """x crossing one word, three words, exactly one word (a second VERTEX word) and one voxel more; the boxes of the raster's test of the
    same name; arbitrary bits (NaN and -0 included); all four contours in one call and single ones; both rules, both kernel forms, the
    volume layouts in turn."""
    state = mc.arbitrary_bits(shape, seed=23)
    m = orf.members(state)
    assert np.isnan(state).any() and (vt.bits(state) == 0x80000000).any()
    seen = 0
    for n, box in enumerate(oc.edge_boxes(shape)):
        ctx.set_volume_layout((0, 3, 1)[n % 3])
        ctx.volume_upload(0, state)
        calls = [desc(shape, CT, box, (488, 488), contours=15, connect=connect) for connect in (capi.OUTLINE_SPLIT, capi.OUTLINE_JOIN)]
        calls.append(desc(shape, CT, box, (0, 976), contours=1 << (n % 4), connect=n % 2))
        for d in calls:
            want = reference(d, m)
            for flavour in (0, 1):
                ctx.set_kernel_flavour(flavour)
                _, _, res, _, _ = check(ctx, d, m, what=(box, flavour, d.connect, d.contours), want=want)
                seen = max(seen, res.n_polygons)
    assert seen > 16  # (not vacuous)


def test_saddles(ctx):
    """A checkerboard (every interior vertex is a saddle) and a random mask of p = 0.5 at 64 x 130, under both rules."""
    shape = (2, 130, 64)
    board = np.broadcast_to((np.add.outer(np.arange(130), np.arange(64)) & 1) == 0, (4,) + shape).copy()
    rand = oc.random_members(shape, 0.5, 5)
    for name, m in (("checkerboard", board), ("random", rand)):
        ctx.volume_upload(0, oc.volume(m, seed=6))
        for connect in (capi.OUTLINE_SPLIT, capi.OUTLINE_JOIN):
            d = desc(shape, oc.GRIDS[2], None, (250, 699), contours=0b0011, connect=connect)
            want = reference(d, m)
            for flavour in (0, 1):
                ctx.set_kernel_flavour(flavour)
                _, _, res, _, _ = check(ctx, d, m, what=(name, connect, flavour), want=want)
                if name == "checkerboard" and connect == capi.OUTLINE_SPLIT:
                    assert res.n_polygons == 2 * 2 * 130 * 32 and res.n_points == 4 * res.n_polygons  # every voxel on its own


@pytest.mark.parametrize("p,connect", [(0.6, capi.OUTLINE_SPLIT), (0.5, capi.OUTLINE_JOIN)], ids=["split_p0.6", "join_p0.5"])
def test_long_loops(ctx, p, connect):
    """Random masks at 140 x 140 x 2 whose longest loop has more than a thousand corners: the default form stops after the first round
    that changes nothing, well before the plain form's fixed count, and both give the same output."""
    shape = (2, 140, 140)
    m = oc.random_members(shape, p, 7)
    ctx.volume_upload(0, oc.volume(m, seed=8))
    d = desc(shape, CT, None, (488, 488), connect=connect)
    ctx.set_kernel_flavour(0)
    a_pts, a_polys, a_res, a_cnt, want = check(ctx, d, m, False)
    assert want["longest"] >= 1024, want["longest"]
    ctx.set_kernel_flavour(1)
    b_pts, b_polys, b_res, b_cnt, plain = check(ctx, d, m, True)
    assert np.array_equal(a_pts, b_pts) and a_polys == b_polys and a_res.as_tuple() == b_res.as_tuple()
    assert b_cnt[2] == plain["rounds"] == int(np.ceil(np.log2(b_cnt[0]))) and a_cnt[2] == want["rounds"]
    assert a_cnt[2] < b_cnt[2], (a_cnt, b_cnt)


def test_index_edges(ctx):
    """65535 voxels along x (1024 voxel words, 1024 vertex words) and along y (65536 vertex rows) with an alternating pattern, and
    coordinates at the ends of the range: the last vertex exactly on +-2^29 is traced, one step further is refused."""
    top = 1 << 29
    for shape in ((1, 2, 65535), (1, 65535, 2)):
        nz, ny, nx = shape
        m = np.zeros((4,) + shape, bool)
        m[0, 0] = (np.add.outer(np.arange(ny), np.arange(nx)) % 3) != 1
        m[3, 0] = (np.add.outer(np.arange(ny), np.arange(nx)) & 1) == 0
        ctx.volume_upload(0, oc.volume(m, seed=9))
        sp = (8192, 3) if nx > ny else (3, 8192)
        long_axis = 0 if nx > ny else 1
        for sign in (1, -1):
            # the last (sign = 1) or first (sign = -1) vertex of the long axis exactly on sign * 2^29
            origin = [100, 100]
            origin[long_axis] = top - max(nx, ny) * 8192 + 5 if sign == 1 else -top + 5
            d = desc(shape, (sp, tuple(origin)), None, tuple(5 if a == long_axis else 0 for a in range(2)), contours=0b1001, connect=(sign + 1) // 2)
            want = reference(d, m)
            for flavour in (0, 1):
                ctx.set_kernel_flavour(flavour)
                pts, _, res, _, _ = check(ctx, d, m, what=(shape, sign, flavour), want=want)
                assert pts[:, long_axis].max() == top if sign == 1 else pts[:, long_axis].min() == -top
                assert res.n_points > 65535
            origin[long_axis] += sign
            bad = d.copy(origin=origin, max_points=0, max_polygons=0)
            assert ctx.lib.vr_mask_outlines(ctx.h, C.byref(bad), None) == capi.VR_ERR_INVALID_ARG
            assert b"2^29" in ctx.lib.vr_last_error(ctx.h)


@pytest.mark.parametrize("grid,offset", [(CT, (488, 488)), (oc.GRIDS[0], (0, 0))], ids=["ct_offset488", "unit_offset0"])
def test_round_trip_on_the_device(ctx, grid, offset):
    """Trace -> vr_mask_polygons EVEN_ODD / REPLACE into another slot: the downloaded components are 1.0f exactly where the source's are
    members, under both connect rules, over the whole volume and over a box that cuts the structures."""
    shape = (5, 37, 130)
    m = oc.blobs(shape, seed=12)
    m[3] = oc.random_members(shape, 0.5, 13)[3]
    ctx.volume_upload(0, oc.volume(m, seed=14))
    for box in (mc.whole(shape), ((3, 2, 1), (127, 30, 4))):
        inbox = np.zeros(shape, bool)
        inbox[box[0][2]:box[1][2], box[0][1]:box[1][1], box[0][0]:box[1][0]] = True
        for connect in (capi.OUTLINE_SPLIT, capi.OUTLINE_JOIN):
            ctx.volume_upload(1, mc.arbitrary_bits(shape, seed=15))
            pts, polys, res, _, _ = check(ctx, desc(shape, grid, box, offset, contours=15, connect=connect), m, False, (box, connect))
            p = capi.PolygonsDesc()
            p.grid_slot, p.dst_slot, p.contours, p.rule, p.combine = 0, 1, 15, capi.POLY_EVEN_ODD, capi.MORPH_REPLACE
            back = ctx.mask_polygons(p.copy(box_lo=box[0], box_hi=box[1], spacing=grid[0], origin=grid[1]), pts, polys)
            got = ctx.volume_download(1, shape)
            for k in range(4):
                assert np.array_equal(vt.bits(got[..., k])[inbox], np.where(m[k], 0x3F800000, 0).astype(np.uint32)[inbox]), (box, connect, k)
                assert back.voxels[k] == int((m[k] & inbox).sum()) == res.area2[k] // 2


def test_composition_with_grow_and_morph(ctx):
    """vr_segment_grow -> vr_mask_morph dilate -> trace equals the restatement on the downloaded mask."""
    shape = (9, 37, 70)
    nz, ny, nx = shape
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    value = np.zeros(shape + (4,), f32)
    value[..., 3] = np.sin(0.31 * x) * np.cos(0.23 * y) + 0.1 * z  # ridges and saddles around the seed
    ctx.volume_upload(0, value)
    ctx.volume_upload(1, np.zeros(shape + (4,), f32))
    grown = ctx.segment_grow(ctx.grow_whole(0, 1, 0, -0.2, 9.0).copy(seeds=[(5, 0, 4)]))
    ctx.mask_morph(ctx.morph_whole(1, 0, 1, 1, capi.MORPH_DILATE))
    m = orf.members(ctx.volume_download(1, shape))
    assert 500 < grown.voxels < m[1].sum() < nx * ny * nz and m[0].sum() == grown.voxels
    for connect in (capi.OUTLINE_SPLIT, capi.OUTLINE_JOIN):
        _, _, res, _, _ = check(ctx, desc(shape, CT, None, (488, 488), src_slot=1, contours=0b0011, connect=connect), m, what=connect)
        assert res.area2[0] == 2 * grown.voxels and res.polygons_of[0] >= nz and res.polygons_of[1] >= nz


def test_side_effects():
    """The call writes no slot and disturbs nothing: the slots' bits, a rendered frame, vr_last_counters and what the other tools report
    are the same before and after."""
    n = 16
    variant = capi.VOLUME_MASK
    vols, tfs = vt.scene(variant, n)
    shape = vols[0].shape[:3]
    step, count = hr.stepping_params(n, n, n)
    u = hr.make_uniforms(W, H, steps_count=count, step_size=step)
    with capi.Context(W, H, 0) as c:
        frame, _, _ = vt.gpu_render(c, variant, u, vols, tfs)
        c.mask_morph(c.morph_whole(0, 0, 0, 1, capi.MORPH_DILATE))
        c.render(variant)
        frame = c.download()[0]

        def reports():
            return (c.counters(), c.last_kernel_flavour(), len(c.kernel_times()), c.grow_counters(), c.grow_timing(), c.morph_counters(),
                    c.morph_timing(), c.dist_counters(), c.dist_timing(), c.polygons_counters(), c.polygons_timing())

        earlier = reports()
        before = [c.volume_download(s, vols[s].shape[:3]) for s in range(len(vols))]
        assert c.outlines_counters() == (0, 0, 0) and c.outlines_timing() == (0.0, 0.0, 0.0, 0.0)
        _, _, res, cnt, _ = check(c, c.outlines_whole(0).copy(contours=0b0011), orf.members(before[0]))
        assert res.n_polygons > 0 and cnt[2] > 0
        timing = c.outlines_timing()
        assert len(timing) == 4 and all(t > 0.0 for t in timing)
        assert reports() == earlier
        for s in range(len(vols)):
            assert np.array_equal(vt.bits(c.volume_download(s, vols[s].shape[:3])), vt.bits(before[s]))
        assert np.array_equal(vt.bits(c.download()[0]), vt.bits(frame))
        c.render(variant)
        assert np.array_equal(vt.bits(c.download()[0]), vt.bits(frame))
        assert (c.counters(), c.last_kernel_flavour()) == earlier[:2]


def raw(ctx, d, n_points, n_polygons, sentinel=0x5A):
    """One raw vr_mask_outlines with buffers of the given capacities, pre-filled with a sentinel: (rc, points, polygons, result)."""
    pts = np.full((max(n_points, 1), 2), sentinel, np.int32)
    polys = (capi.Polygon * max(n_polygons, 1))()
    C.memset(polys, sentinel, C.sizeof(polys))
    full = d.copy(max_points=n_points, max_polygons=n_polygons, points=pts.ctypes.data if n_points else None,
                  polygons=C.cast(polys, C.c_void_p).value if n_polygons else None)
    res = capi.OutlinesResult()
    rc = ctx.lib.vr_mask_outlines(ctx.h, C.byref(full), C.byref(res))
    return rc, pts, bytes(polys), res


def test_capacity(ctx):
    shape = (3, 20, 70)
    m = oc.blobs(shape, seed=21)
    ctx.volume_upload(0, oc.volume(m, seed=22))
    d = desc(shape, CT, None, (488, 488), contours=0b0110)
    want = orf.trace(m, 0b0110, 0, *mc.whole(shape), CT[1], CT[0], (488, 488))
    n, q = want["result"][:2]
    assert n > 50 and q > 5
    rc, pts, polys, res = raw(ctx, d, 0, 0)  # the counting call
    assert rc == capi.VR_OK and res.as_tuple() == want["result"] and ctx.outlines_counters()[:2] == (n, q)
    rc, pts, polys, res = raw(ctx, d, n, q)  # exact capacity
    assert rc == capi.VR_OK and res.as_tuple() == want["result"] and np.array_equal(pts, want["points"])
    assert [(g.first, g.count, g.slice, g.contour) for g in (capi.Polygon * q).from_buffer_copy(polys)] == want["polygons"]
    rc, pts, polys, res = raw(ctx, d, n + 7, q + 3)  # more than needed: the rest keeps the sentinel
    assert rc == capi.VR_OK and np.array_equal(pts[:n], want["points"]) and (pts[n:] == 0x5A).all() and polys[16 * q:] == b"\x5a" * 48
    for cap in ((n - 1, q), (n, q - 1), (0, q), (n, 0), (1, 1)):  # one point short, one polygon short, one buffer missing
        rc, pts, polys, res = raw(ctx, d, *cap)
        assert rc == capi.VR_ERR_INVALID_ARG, cap
        err = ctx.lib.vr_last_error(ctx.h).decode()
        assert err.startswith("vr_mask_outlines") and str(n) in err and str(q) in err, err
        assert (pts == 0x5A).all() and polys == b"\x5a" * len(polys), cap
        assert res.as_tuple() == want["result"], cap
    check(ctx, d, m)  # (the context is usable)


def test_argument_errors_leave_the_context_usable(ctx):
    shape = (4, 12, 70)
    nz, ny, nx = shape
    m = oc.blobs(shape, seed=31)
    ctx.volume_upload(0, oc.volume(m, seed=32))
    good = desc(shape, CT, None, (488, 488), contours=0b0101)
    check(ctx, good, m)
    counters = ctx.outlines_counters()
    top = 1 << 29
    pts = np.zeros((4, 2), np.int32)
    polys = (capi.Polygon * 1)()
    invalid = [dict(src_slot=-1), dict(src_slot=3), dict(contours=0), dict(contours=16), dict(contours=-1), dict(connect=-1), dict(connect=2),
               dict(box_lo=(-1, 0, 0)), dict(box_hi=(nx + 1, ny, nz)), dict(box_hi=(nx, ny, nz + 1)), dict(box_lo=(5, 0, 0), box_hi=(4, ny, nz)),
               dict(spacing=(0, 977)), dict(spacing=(977, 0)), dict(spacing=((1 << 20) + 1, 977)), dict(spacing=(977, (1 << 20) + 1)),
               dict(offset=(977, 0)), dict(offset=(0, 977)), dict(offset=(0xFFFFFFFF, 0)),
               dict(origin=(top + 1, 0)), dict(origin=(0, -top - 1)), dict(origin=(top - 69 * 977, 0)), dict(origin=(0, -top + 487)),
               dict(max_points=4), dict(max_polygons=1), dict(points=pts.ctypes.data), dict(polygons=C.cast(polys, C.c_void_p).value)]
    for over in invalid:
        d = good.copy(**over)
        assert ctx.lib.vr_mask_outlines(ctx.h, C.byref(d), C.byref(capi.OutlinesResult())) == capi.VR_ERR_INVALID_ARG, over
        assert (ctx.lib.vr_last_error(ctx.h) or b"").decode().startswith("vr_mask_outlines"), over
    assert ctx.lib.vr_mask_outlines(ctx.h, None, None) == capi.VR_ERR_INVALID_ARG
    assert ctx.lib.vr_mask_outlines(None, C.byref(good), None) == capi.VR_ERR_INVALID_ARG
    assert ctx.lib.vr_outlines_counters(ctx.h, None) == capi.VR_ERR_INVALID_ARG
    assert ctx.lib.vr_outlines_timing(ctx.h, None) == capi.VR_ERR_INVALID_ARG
    assert ctx.outlines_counters() == counters
    # the extreme vertices exactly on the range are fine
    check(ctx, good.copy(origin=(top - 70 * 977 + 488, -top + 488)), m)
    with capi.Context(W, H, 0) as empty:
        assert empty.lib.vr_mask_outlines(empty.h, C.byref(good), None) == capi.VR_ERR_NOT_READY
        err = empty.lib.vr_last_error(empty.h)
        assert err.startswith(b"vr_mask_outlines") and b"empty" in err
        assert empty.lib.vr_outlines_whole(empty.h, 0, C.byref(capi.OutlinesDesc())) == capi.VR_ERR_NOT_READY
    # vr_outlines_whole
    assert bytes(ctx.outlines_whole(0)) == bytes(desc(shape))
    for bad in (3, -1):
        assert ctx.lib.vr_outlines_whole(ctx.h, bad, C.byref(capi.OutlinesDesc())) == capi.VR_ERR_INVALID_ARG
    assert ctx.lib.vr_outlines_whole(ctx.h, 0, None) == capi.VR_ERR_INVALID_ARG
    # a NULL result is fine; an empty box and an empty contour give no polygons
    assert ctx.lib.vr_mask_outlines(ctx.h, C.byref(good), None) == capi.VR_OK
    for box in (((3, 2, 1), (3, 9, 3)), ((0, 0, 2), (nx, ny, 2))):
        _, polys_, res, cnt, _ = check(ctx, desc(shape, CT, box, contours=15), m, what=box)
        assert polys_ == [] and res.as_tuple() == EMPTY and cnt == (0, 0, 0)
    some = m & np.array([1, 0, 1, 0], bool)[:, None, None, None]
    ctx.volume_upload(0, oc.volume(some, seed=33))
    _, polys_, res, cnt, _ = check(ctx, desc(shape, CT, contours=0b1010), some)
    assert polys_ == [] and res.as_tuple() == EMPTY and cnt == (0, 0, 0)


def test_timing_and_counters_of_every_ending(ctx):
    """What vr_outlines_timing and vr_outlines_counters report after each ending a small input reaches, on (5, 12, 30) voxels with one
    non-empty contour: a phase the call never began is exactly 0.0, one it began is timed; the counters are the call's own; an
    argument error leaves both as they were."""
    shape = (5, 12, 30)
    nz, ny, nx = shape
    m = oc.blobs(shape, seed=51)
    m[1:] = False
    ctx.volume_upload(0, oc.volume(m, seed=52))
    d = desc(shape, CT, None, (488, 488))
    part = desc(shape, CT, ((2, 1, 1), (nx, ny - 2, 3)), (488, 488))
    (n, q), (n2, q2) = (reference(x, m)["result"][:2] for x in (d, part))
    assert n > 8 and q > 1 and 0 < n2 < n

    def ended(call, rc, began, counted, what):
        got = call[0]
        ms, cnt = ctx.outlines_timing(), ctx.outlines_counters()
        assert got == rc, (what, got)
        assert all(t > 0.0 for t in ms[:began]) and ms[began:] == (0.0,) * (4 - began), (what, ms)
        assert cnt[:2] == counted and (cnt[2] > 0) == (counted != (0, 0)), (what, cnt)

    def argument_error(what):
        before = ctx.outlines_timing(), ctx.outlines_counters()
        assert raw(ctx, d.copy(contours=16), n, q)[0] == capi.VR_ERR_INVALID_ARG
        assert (ctx.outlines_timing(), ctx.outlines_counters()) == before, what

    ended(raw(ctx, d, n, q), capi.VR_OK, 4, (n, q), "exact capacity")
    argument_error("after a full call")
    ended(raw(ctx, desc(shape, CT, ((3, 2, 1), (3, 9, 3)), (488, 488)), n, q), capi.VR_OK, 0, (0, 0), "empty box")
    argument_error("after an empty box")
    ended(raw(ctx, part, 0, 0), capi.VR_OK, 4, (n2, q2), "counting call")
    ended(raw(ctx, d.copy(contours=0b0010), n, q), capi.VR_OK, 2, (0, 0), "contour empty in the box")
    argument_error("after a call without a corner")
    ended(raw(ctx, d, n - 1, q), capi.VR_ERR_INVALID_ARG, 4, (n, q), "one point short")
    ended(raw(ctx, part, n2, q2 - 1), capi.VR_ERR_INVALID_ARG, 4, (n2, q2), "one polygon short")
    argument_error("after a buffer too small")


SWEEP = oc.sweep(40)


@pytest.mark.parametrize("i", range(40))
def test_random_sweep(ctx, i):
    case = SWEEP[i]
    ctx.set_kernel_flavour(1 if case["plain"] else 0)
    ctx.volume_upload(i % 3, oc.volume(case["m"], seed=case["seed"]))
    d = capi.OutlinesDesc().copy(src_slot=i % 3, contours=case["contours"], connect=case["connect"], box_lo=case["box_lo"], box_hi=case["box_hi"],
                                 origin=case["origin"], spacing=case["spacing"], offset=case["offset"])
    check(ctx, d, case["m"], case["plain"], what=i)


def test_application_mask_to_contours(tmp_path):
    """MaskToContours -> vrh_struct_from_contours -> ContoursToMask reproduces the mask on a grid of 0.977 x 0.977 x 2.5 mm off a negative
    origin read from (synthetic) DICOM.  The millimetre floats round back to the same micrometres there: every coordinate is below
    2^24 um, so its float32 millimetres are within half a micrometre of it and llround(v * 1000.0) returns it."""
    import dicom_writer as dw
    from volumerendering_amd import host, synth
    n, nz = 40, 12
    raw_ct = synth.ct_phantom_raw(n)[:nz]
    d = tmp_path / "ct"
    d.mkdir()
    x0, y0, z0 = -19.5, -12.25, 10.0
    for k in range(nz):
        dw.write_slice(str(d / f"{k:03d}.dcm"), raw_ct[k], rows=n, cols=n, instance=k + 1, position=(x0, y0, z0 + 2.5 * k), spacing=(0.977, 0.977),
                       thickness=2.5, largest=int(raw_ct.max()), frame_uid="1.2.840.7")
    grid = host.VolumeFile.from_dicom(str(d))
    shape = (nz, n, n)
    m = oc.blobs(shape, seed=41, n=3)
    m[1] = oc.random_members(shape, 0.5, 42)[1]
    m[3] = False
    origin, spacing, offset = (-19500, -12250), (977, 977), (488, 488)
    with host.Application(W, H, 0) as app:
        app.OnStart(capi.BASIC, [grid])
        c = app.context()
        c.volume_upload(1, oc.volume(m, seed=43))
        for connect in (capi.OUTLINE_SPLIT, capi.OUTLINE_JOIN):
            want = orf.trace(m, 0b0111, connect, *mc.whole(shape), origin, spacing, offset)
            # MaskOutlines is vr_mask_outlines on the application's context
            dsc = c.outlines_whole(1).copy(contours=0b0111, connect=connect, origin=origin, spacing=spacing, offset=offset)
            pts, polys, res = app.mask_outlines(dsc)
            assert np.array_equal(pts, want["points"]) and polys == want["polygons"] and res.as_tuple() == want["result"]
            structures = app.mask_to_contours(1, 0b0111, connect, grid)
            got = structures.contours()
            assert len(got) == 3 and [len(g) for g in got] == list(want["result"][2][:3])
            flat = [p for g in got for p in g]
            assert np.abs(want["points"]).max() < 1 << 24
            for poly, (first, count, z, k) in zip(flat, want["polygons"]):
                q = poly.reshape(-1, 3)
                um = np.round(q[:, :2].astype(np.float64) * 1000.0).astype(np.int64)
                assert np.array_equal(um, want["points"][first:first + count]) and (q[:, 2] == f32(z0) + f32(z) * f32(2.5)).all()
            # back into a mask: (the last structure of a file cannot be selected: Create3DMask's rule)
            again = host.StructureFile.from_contours(got + [[np.zeros(3, f32)]], frame_of_reference="1.2.840.7")
            back = app.contours_to_mask(again, [1, 2, 3, 0], grid, 2)
            out = c.volume_download(2, shape)
            for k in range(3):
                assert np.array_equal(vt.bits(out[..., k]), np.where(m[k], 0x3F800000, 0).astype(np.uint32)), (connect, k)
                assert back.voxels[k] == int(m[k].sum())
        with pytest.raises(capi.VrError) as e:
            app.mask_to_contours(1, 0, 0, grid)
        assert e.value.code == capi.VR_ERR_INVALID_ARG
        with pytest.raises(capi.VrError):
            app.mask_to_contours(1, 1, 0, host.VolumeFile.from_raw(raw_ct))  # (not read from DICOM: no spacing)
