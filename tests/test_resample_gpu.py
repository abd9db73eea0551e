"""GPU side of the resampling tool (vr_volume_resample, csrc/vr_resample.h): the downloaded destination slot EQUAL, bit for bit, to the
numpy restatement (resample_ref.py, pinned on the CPU by tests/test_resample.py), and the result, out[0] and out[1] + out[2] == out[0]
too -- wavefront-unit edges and boxes, every transform, both filters, the channel sets, both arithmetic modes, both kernel forms,
the volume layouts, hostile values, what the default form settles, the index edges, the errors, the freshness of everything
downstream, a random sweep, and the host surface.  (Where a stored value comes out of the lerps and the restatement has a NaN, a NaN
is asked for: an arithmetic NaN has no defined payload, as in the slice tests.  Copies -- NEAREST, `outside`, what is not written --
are compared in every bit.)"""
import ctypes as C

import numpy as np
import pytest

import hist_ref as hh
import host_ref as hr
import resample_cases as rc
import resample_ref as rr
import vrtest as vt
from volumerendering_amd import capi

pytestmark = pytest.mark.gpu
f32 = np.float32
W, H = 64, 48
MAIN = rc.SRC_SHAPES[0]
FILTERS = [capi.RESAMPLE_LINEAR, capi.RESAMPLE_NEAREST]
ARITH = [capi.ARITH_SEPARATE, capi.ARITH_FUSED]


def desc(dst_shape, geom, box=None, **over):
    """A descriptor from slot 0 into slot 1: all four components, LINEAR, outside = (7, -2, 0.5, -0), the whole grid unless a box is given."""
    n = rc.n_of(dst_shape)
    lo, hi = box if box else ((0, 0, 0), n)
    o, di, dj, dk = geom
    base = dict(src_slot=0, dst_slot=1, channels=15, filter=capi.RESAMPLE_LINEAR, dst_n=n, origin=o, di=di, dj=dj, dk=dk,
                outside=(7.0, -2.0, 0.5, -0.0), box_lo=lo, box_hi=hi)
    return capi.ResampleDesc().copy(**{**base, **over})


def check(ctx, d, src, before, fused=False, what=None):
    """One vr_volume_resample against the restatement: the destination slot, the result, out[0] and out[1] + out[2] == out[0].  `src`:
    the source slot's voxels; `before`: the destination's before the call (None: an empty slot).  Returns (result, counters, the
    downloaded destination, the restatement's result)."""
    ctx.set_arithmetic(capi.ARITH_FUSED if fused else capi.ARITH_SEPARATE)
    res = ctx.volume_resample(d)
    cnt = ctx.resample_counters()
    nx, ny, nz = tuple(d.dst_n)
    got = ctx.volume_download(d.dst_slot, (nz, ny, nx))
    want, want_res, box, copied = rr.resample_desc(src, before, d, fused)
    if not rr.same(got, want, copied):
        bad = np.argwhere((vt.bits(got) != vt.bits(want)) & ~(np.isnan(want) & ~copied & np.isnan(got)))
        raise AssertionError((what, len(bad), bad[:4], got[tuple(bad[0][:3])], want[tuple(bad[0][:3])]))
    assert res.as_tuple() == want_res, (what, res.as_tuple(), want_res)
    assert cnt[0] == box and cnt[1] + cnt[2] == cnt[0], (what, cnt, box)
    return res, cnt, got, want_res


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


@pytest.mark.parametrize("src_shape", rc.SRC_SHAPES, ids=["70x9x5", "1x7x6", "1x1x1"])
def test_shapes_and_boxes(ctx, src_shape):
    """Destinations whose x crosses two wavefront units with a tail, is exactly one unit, and is one voxel over; boxes aligned to nothing,
    empty and of one voxel; into a destination of arbitrary bits, whose untouched voxels and unselected components keep theirs; both
    kernel forms.  The rotation leaves voxels inside and outside on every pair of shapes."""
    src = rc.hostile(src_shape, 11)
    ctx.volume_upload(0, src)
    for dst_shape in rc.DST_SHAPES:
        state = rc.arbitrary_bits(dst_shape, 12)
        ctx.volume_upload(1, state)
        geom = rc.transform("rot30z", src_shape, dst_shape)
        for k, box in enumerate(rc.boxes(dst_shape)):
            for channels in (15, 5):
                for flavour in (0, 1):
                    ctx.set_kernel_flavour(flavour)
                    d = desc(dst_shape, geom, box, channels=channels, filter=FILTERS[k % 2])
                    res, cnt, state, want = check(ctx, d, src, state, what=(dst_shape, box, channels, flavour))
                    if flavour == 1:
                        assert cnt[1] == res.inside and cnt[2] == res.outside
                    if k == 0:
                        assert want[0] > 0 and want[1] > 0


@pytest.mark.parametrize("dst_shape", rc.DST_SHAPES, ids=["130x6x7", "64x5x3", "65x1x2"])
def test_an_empty_destination_is_created(dst_shape):
    """An empty slot gets dst_n and +0.0f in every component that is not written and every voxel outside the box; an empty box still
    creates it."""
    src = rc.volume(MAIN, 13)
    geom = rc.transform("magnify4", MAIN, dst_shape)
    for box in rc.boxes(dst_shape)[1:3]:
        with capi.Context(W, H, 0) as c:
            c.volume_upload(0, src)
            d = desc(dst_shape, geom, box, dst_slot=2, channels=10)
            _, _, got, _ = check(c, d, src, None, what=(dst_shape, box))
            assert not vt.bits(got[..., [0, 2]]).any()
            check(c, d.copy(channels=5, box_lo=(0, 0, 0), box_hi=rc.n_of(dst_shape)), src, got)  # (now a filled one of exactly dst_n)


@pytest.mark.parametrize("fused", [False, True], ids=["separate", "fused"])
@pytest.mark.parametrize("name", rc.BOTH + rc.ALL_INSIDE + rc.ALL_OUTSIDE)
def test_transforms(ctx, name, fused):
    """A 4 x magnification with a sub-voxel offset, a 3 x minification, a 30 degree rotation about z and one about an oblique axis with part
    of the grid outside, di = dj = dk = 0, an origin with a NaN and one at 1e30; both filters, both kernel forms."""
    src = rc.volume(MAIN, 21)
    ctx.volume_upload(0, src)
    for dst_shape in rc.DST_SHAPES:
        state = rc.arbitrary_bits(dst_shape, 22)
        ctx.volume_upload(1, state)
        geom = rc.transform(name, MAIN, dst_shape)
        for filt in FILTERS:
            for flavour in (0, 1):
                ctx.set_kernel_flavour(flavour)
                res, cnt, state, want = check(ctx, desc(dst_shape, geom, filter=filt), src, state, fused, what=(name, dst_shape, filt, flavour))
                assert (want[0] > 0) == (name not in rc.ALL_OUTSIDE) and (want[1] > 0) == (name not in rc.ALL_INSIDE), (name, want)
                if name in rc.ALL_OUTSIDE:
                    assert cnt[1] == 0


@pytest.mark.parametrize("fused", [False, True], ids=["separate", "fused"])
@pytest.mark.parametrize("filt", FILTERS, ids=["linear", "nearest"])
def test_identity_law(ctx, filt, fused):
    """The power-of-two identity reproduces the uploaded source bit for bit (tests/test_resample.py: the law), in both forms and layouts."""
    src = rc.volume(rc.POW2, 5)
    ctx.volume_upload(0, src)
    ctx.set_arithmetic(capi.ARITH_FUSED if fused else capi.ARITH_SEPARATE)
    for layout in (0, 3):
        for flavour in (0, 1):
            ctx.set_volume_layout(layout)
            ctx.set_kernel_flavour(flavour)
            ctx.volume_upload(1, rc.arbitrary_bits(rc.POW2, 6))
            d = ctx.resample_identity(0, 1, filt)
            n, o, di, dj, dk = rr.identity(rc.POW2)
            assert bytes(d) == bytes(desc(rc.POW2, (o, di, dj, dk), filter=filt, outside=(0, 0, 0, 0)))
            res = ctx.volume_resample(d)
            assert np.array_equal(vt.bits(ctx.volume_download(1, rc.POW2)), vt.bits(src)), (layout, flavour)
            assert res.as_tuple() == (8 * 16 * 32, 0, (0, 0, 0), (8, 16, 32)) and ctx.resample_counters() == (4096, 4096, 0)


@pytest.mark.parametrize("layout", [0, 3], ids=["bricked", "linear"])
@pytest.mark.parametrize("channels", rc.CHANNELS)
def test_variants_with_hostile_values(ctx, channels, layout):
    """Every channel set in both filters, arithmetic modes, kernel forms and layouts: a source with NaN, +-inf, -0 and denormals, hostile
    `outside` values, a destination of arbitrary bits."""
    src = rc.hostile(MAIN, 31)
    dst_shape = rc.DST_SHAPES[0]
    state = rc.arbitrary_bits(dst_shape, 32)
    ctx.set_volume_layout(layout)
    ctx.volume_upload(0, src)
    ctx.volume_upload(1, state)
    for name in ("oblique", "magnify4"):
        geom = rc.transform(name, MAIN, dst_shape)
        for filt in FILTERS:
            for fused in (False, True):
                outs = []
                for flavour in (0, 1):
                    ctx.set_kernel_flavour(flavour)
                    d = desc(dst_shape, geom, channels=channels, filter=filt, outside=rc.HOSTILE_OUTSIDE)
                    res, cnt, state, _ = check(ctx, d, src, state, fused, what=(name, channels, filt, fused, flavour, layout))
                    outs.append((vt.bits(state).copy(), res.as_tuple(), cnt[0]))
                    if flavour == 1:
                        assert cnt[1] == res.inside
                same = ~(np.isnan(outs[0][0].view(f32)) & np.isnan(outs[1][0].view(f32)))
                assert np.array_equal(outs[0][0][same], outs[1][0][same]) and outs[0][1:] == outs[1][1:]


@pytest.mark.parametrize("fused", [False, True], ids=["separate", "fused"])
def test_settling(ctx, fused):
    """A source with bricks of a non-zero constant, of +0, of mixed +-0, one NaN voxel and a noisy region, channel 3 alone: the two forms
    store the same bits, the default form stores more voxels without a load than the plain one (whose out[2] is exactly the outside
    voxels), and the layouts agree."""
    src = rc.settle_source()
    dst_shape = (6, 7, 650)
    s = (rc.n_of(src.shape[:3]), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    dgrid = (rc.n_of(dst_shape), (-4.3, -0.7, -1.1), (88.0 / 650, 17.0 / 7, 18.0 / 6))
    geom = rr.between(*s, *dgrid)
    ctx.volume_upload(0, src)
    for layout in (0, 3):
        ctx.set_volume_layout(layout)
        outs = {}
        for flavour in (0, 1):
            ctx.set_kernel_flavour(flavour)
            ctx.volume_upload(1, rc.arbitrary_bits(dst_shape, 41))
            d = desc(dst_shape, geom, channels=8, outside=(0, 0, 0, -1.0))
            res, cnt, got, want = check(ctx, d, src, rc.arbitrary_bits(dst_shape, 41), fused, what=(layout, flavour))
            outs[flavour] = (vt.bits(got), res.as_tuple(), cnt)
        assert np.array_equal(outs[0][0], outs[1][0]) and outs[0][1] == outs[1][1] and outs[0][2][0] == outs[1][2][0]
        inside, outside = outs[1][1][0], outs[1][1][1]
        assert inside > 0 and outside > 0
        assert outs[1][2][1] == inside and outs[1][2][2] == outside
        assert outs[0][2][2] > outs[1][2][2], (outs[0][2], outs[1][2])
        # NEAREST and a launch of all four components do not settle: they load every inside voxel in the default form too
        ctx.set_kernel_flavour(0)
        state = outs[1][0].view(f32)
        for over in (dict(filter=capi.RESAMPLE_NEAREST), dict(channels=15)):
            d = desc(dst_shape, geom, **{**dict(channels=8, outside=(0, 0, 0, -1.0)), **over})
            res, cnt, state, _ = check(ctx, d, src, state, fused)
            assert cnt[1] == res.inside
    # the records follow the source: noise uploaded into the slot settles nothing, the source again settles as before
    ctx.set_volume_layout(0)
    d = desc(dst_shape, geom, channels=8, outside=(0, 0, 0, -1.0))
    noise = rc.volume(src.shape[:3], 42)
    for vol in (noise, src):
        ctx.volume_upload(0, vol)
        res, cnt, state, _ = check(ctx, d, vol, state, fused)
        assert (cnt[1] == res.inside) == (vol is noise)


def test_index_edges(ctx):
    """A destination of 65535 x 1 x 2 from a small source, and a source of 65535 x 2 x 1 onto a small destination."""
    src = rc.volume(MAIN, 51)
    long_shape = (2, 1, 65535)
    state = rc.arbitrary_bits(long_shape, 52)
    ctx.volume_upload(0, src)
    ctx.volume_upload(1, state)
    s = (rc.n_of(MAIN), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    geom = rr.between(*s, rc.n_of(long_shape), (-3.0, 2.2, 1.4), (76.0 / 65535, 1.0, 2.0))
    for flavour in (0, 1):
        ctx.set_kernel_flavour(flavour)
        for box in (None, ((62490, 0, 1), (62555, 1, 2))):  # the whole grid (1024 units per row), then 65 voxels across the source's far face
            res, _, state, want = check(ctx, desc(long_shape, geom, box, channels=8 if box else 15), src, state, what=(flavour, box))
            assert want[0] > 0 and want[1] > 0
    big = rc.volume((1, 2, 65535), 53)
    ctx.volume_upload(0, big)
    dst_shape = rc.DST_SHAPES[0]
    s = ((65535, 2, 1), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    geom = rr.between(*s, rc.n_of(dst_shape), (65400.3, -0.4, -0.2), (1.1, 0.3, 0.1))  # the far end of the long axis, and beyond it
    for filt in FILTERS:
        for layout in (0, 3):
            ctx.set_volume_layout(layout)
            ctx.volume_upload(1, rc.arbitrary_bits(dst_shape, 54))
            res, _, _, want = check(ctx, desc(dst_shape, geom, filter=filt), big, rc.arbitrary_bits(dst_shape, 54), what=(filt, layout))
            assert want[0] > 0 and want[1] > 0


def test_a_source_of_four_gib():
    """A source of 512 x 512 x 1032 voxels, 4.03 GiB: the gathers take their 64-bit addressing, in the bricked and the x-fastest layout,
    and the voxels sampled lie beyond byte 2^32 -- the far corner of a volume that is zero but for its last nine slices."""
    shape = (1032, 512, 512)
    src = np.zeros(shape + (4,), f32)
    src[1023:] = rc.volume((9, 512, 512), 55)
    dst_shape = rc.DST_SHAPES[0]
    s = (rc.n_of(shape), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    geom = rr.between(*s, rc.n_of(dst_shape), (498.3, 504.2, 1023.6), (0.13, 1.4, 1.5))
    state = rc.arbitrary_bits(dst_shape, 56)
    with capi.Context(W, H, 0) as c:
        c.volume_upload(0, src)
        c.volume_upload(1, state)
        for layout in (0, 3):
            c.set_volume_layout(layout)
            for filt in FILTERS:
                for channels in (15, 8):
                    for flavour in (0, 1):
                        c.set_kernel_flavour(flavour)
                        res, cnt, state, want = check(c, desc(dst_shape, geom, channels=channels, filter=filt), src, state, fused=bool(flavour),
                                                      what=(layout, filt, channels, flavour))
                        assert want[0] > 0 and want[1] > 0
        assert np.abs(state[0, 0, :64]).min() > 0.0  # (what was sampled is the band, not the zeros)


def test_errors_leave_the_destination_untouched(ctx):
    src = rc.hostile(MAIN, 61)
    dst_shape = rc.DST_SHAPES[1]
    nx, ny, nz = rc.n_of(dst_shape)
    m = rc.arbitrary_bits(dst_shape, 62)
    ctx.volume_upload(0, src)
    ctx.volume_upload(1, m)
    ctx.volume_upload(2, np.zeros((4, 4, 4, 4), f32))
    good = desc(dst_shape, rc.transform("rot30z", MAIN, dst_shape))
    _, _, m, _ = check(ctx, good, src, m)
    counters = ctx.resample_counters()
    invalid = [dict(src_slot=-1), dict(src_slot=3), dict(dst_slot=-1), dict(dst_slot=3), dict(dst_slot=0), dict(src_slot=1), dict(channels=0),
               dict(channels=16), dict(filter=-1), dict(filter=2), dict(dst_n=(0, ny, nz)), dict(dst_n=(nx, 65536, nz)), dict(dst_n=(nx, ny, -1)),
               dict(dst_n=(nx + 1, ny, nz)), dict(dst_slot=2), dict(box_lo=(-1, 0, 0)), dict(box_hi=(nx + 1, ny, nz)),
               dict(box_hi=(nx, ny, nz + 1)), dict(box_lo=(5, 0, 0), box_hi=(4, ny, nz))]
    for over in invalid:
        d = good.copy(**over)
        assert ctx.lib.vr_volume_resample(ctx.h, C.byref(d), C.byref(capi.ResampleResult())) == capi.VR_ERR_INVALID_ARG, over
        assert (ctx.lib.vr_last_error(ctx.h) or b"").decode().startswith("vr_volume_resample"), over
    assert ctx.lib.vr_volume_resample(ctx.h, None, None) == capi.VR_ERR_INVALID_ARG
    assert ctx.lib.vr_volume_resample(None, C.byref(good), None) == capi.VR_ERR_INVALID_ARG
    assert ctx.lib.vr_resample_counters(ctx.h, None) == capi.VR_ERR_INVALID_ARG
    assert ctx.lib.vr_resample_timing(ctx.h, None) == capi.VR_ERR_INVALID_ARG
    assert ctx.resample_counters() == counters
    assert np.array_equal(vt.bits(ctx.volume_download(1, dst_shape)), vt.bits(m))
    assert np.array_equal(vt.bits(ctx.volume_download(0, MAIN)), vt.bits(src))
    assert np.array_equal(vt.bits(ctx.volume_download(2, (4, 4, 4))), np.zeros((4, 4, 4, 4), np.uint32))
    # no value of origin, di, dj, dk or outside is an error
    wild = good.copy(origin=(float("inf"), float("nan"), -1e38), di=(float("nan"), 1e38, 0), dk=(float("-inf"), 0, 0), outside=rc.HOSTILE_OUTSIDE)
    res, _, m, _ = check(ctx, wild, src, m)
    assert res.inside == 0
    with capi.Context(W, H, 0) as empty:
        assert empty.resample_counters() == (0, 0, 0) and empty.resample_timing() == (0.0, 0.0, 0.0, 0.0)
        assert empty.lib.vr_volume_resample(empty.h, C.byref(good), None) == capi.VR_ERR_NOT_READY
        err = empty.lib.vr_last_error(empty.h)
        assert err.startswith(b"vr_volume_resample") and b"empty" in err
        assert empty.lib.vr_resample_identity(empty.h, 0, 1, 0, C.byref(capi.ResampleDesc())) == capi.VR_ERR_NOT_READY
        with pytest.raises(capi.VrError):  # (the failed call created nothing)
            empty.volume_download(1, dst_shape)
    # vr_resample_identity's arguments
    for bad in ((3, 1, 0), (-1, 1, 0), (0, 3, 0), (0, -1, 0), (0, 0, 0), (0, 1, 2), (0, 1, -1)):
        assert ctx.lib.vr_resample_identity(ctx.h, *bad, C.byref(capi.ResampleDesc())) == capi.VR_ERR_INVALID_ARG, bad
    assert ctx.lib.vr_resample_identity(ctx.h, 0, 1, 0, None) == capi.VR_ERR_INVALID_ARG
    # a NULL result is fine
    assert ctx.lib.vr_volume_resample(ctx.h, C.byref(good), None) == capi.VR_OK


def test_everything_downstream_is_fresh_and_the_other_reports_stay():
    """After a resample into the slot a scene renders, a slice, a histogram and a BASIC frame equal what a fresh upload of the restatement's
    volume gives; what the reporting calls say about the march, the slice, the histogram and the other tools stays."""
    n = 16
    shape = (n, n, n)
    src = np.abs(rc.volume(MAIN, 71)) * f32(0.3)
    old = np.abs(rc.volume(shape, 72)) * f32(0.3)
    tf = (np.linspace(0.0, 1.0, 64).astype(f32), np.tile(np.array([0.8, 0.55, 0.3, 1.0], f32), (64, 1)))
    step, count = hr.stepping_params(n, n, n)
    u = hr.make_uniforms(W, H, steps_count=count, step_size=step)
    with capi.Context(W, H, 0) as c:
        c.volume_upload(0, old)
        c.volume_upload(1, src)
        c.tf_upload(0, *tf)
        c.set_uniforms(vt.to_capi_uniforms(u))
        c.render(capi.BASIC)
        before_frame = c.download()[0]
        hd = c.hist_whole(0, 64, 64.0)
        sd = c.slice_orthogonal(0, 2, n // 2, 1)
        before_hist, before_img = c.histogram(hd), c.slice(sd)
        md = c.morph_whole(0, 0, 0, 1, capi.MORPH_DILATE)
        c.mask_morph(md)
        old = c.volume_download(0, shape)
        c.render(capi.BASIC)

        def reports():
            return (c.counters(), c.last_kernel_flavour(), c.slice_counters(), c.hist_counters(), len(c.kernel_times()), c.grow_counters(),
                    c.morph_counters(), c.morph_timing(), c.dist_counters(), c.components_counters())

        seen = reports()
        d = desc(shape, rc.transform("oblique", MAIN, shape), src_slot=1, dst_slot=0, outside=(0, 0, 0, 0.05))
        res, _, after, _ = check(c, d, src, old)
        assert res.inside > 0 and res.outside > 0
        assert reports() == seen
        timing = c.resample_timing()
        assert len(timing) == 4 and all(t >= 0.0 for t in timing) and timing[1] > 0.0 and timing[3] > 0.0
        hist, img = c.histogram(hd), c.slice(sd)
        c.render(capi.BASIC)
        frame = c.download()[0]
        c.volume_upload(0, after)  # the same context after an upload of the expected volume
        want_hist, want_img = c.histogram(hd), c.slice(sd)
        c.render(capi.BASIC)
        want_frame = c.download()[0]
    assert np.array_equal(hist[0], want_hist[0]) and hist[1] == want_hist[1] and not np.array_equal(hist[0], before_hist[0])
    assert np.array_equal(vt.bits(img), vt.bits(want_img)) and not np.array_equal(vt.bits(img), vt.bits(before_img))
    assert np.array_equal(vt.bits(frame), vt.bits(want_frame)) and not np.array_equal(vt.bits(frame), vt.bits(before_frame))


SWEEP = rc.sweep()


@pytest.mark.parametrize("i", range(len(SWEEP)))
def test_random_sweep(i):
    case = SWEEP[i]
    src = (rc.hostile if case["hostile"] else rc.volume)(case["src_shape"], case["seed"])
    before = None if case["fresh"] else rc.arbitrary_bits(case["dst_shape"], case["seed"] + 1)
    with capi.Context(W, H, 0) as c:
        c.set_kernel_flavour(case["flavour"])
        c.set_volume_layout(case["layout"])
        c.volume_upload(0, src)
        if before is not None:
            c.volume_upload(2, before)
        d = desc(case["dst_shape"], (case["origin"], case["di"], case["dj"], case["dk"]), (case["box_lo"], case["box_hi"]), dst_slot=2,
                 channels=case["channels"], filter=case["filter"], outside=case["outside"])
        check(c, d, src, before, case["fused"], what=case)


def test_application_resample_onto_closes_the_dvh_gap(tmp_path):
    """A CT series and an RTDOSE on a coarser, offset grid read from (synthetic) DICOM, a mask on the CT's grid: the DVH of the dose as
    loaded is VR_ERR_INVALID_ARG (other dimensions); after Application::ResampleOnto into a third slot it equals the restatement's
    resampled dose binned by hist_ref."""
    import dicom_writer as dw
    from volumerendering_amd import host, synth
    n, nz = 40, 12
    raw = synth.ct_phantom_raw(n)[:nz]
    ctd, dsd = tmp_path / "ct", tmp_path / "dose"
    ctd.mkdir()
    dsd.mkdir()
    for k in range(nz):
        dw.write_slice(str(ctd / f"{k:03d}.dcm"), raw[k], rows=n, cols=n, instance=k + 1, position=(-19.0, -20.5, 2.5 * k + 4.0), spacing=(0.977, 0.977),
                       thickness=2.5, largest=int(raw.max()), frame_uid="1.9.9")
    dose_raw = synth.dose_raw(12, 12, 6)
    dw.write_slice(str(dsd / "dose.dcm"), dose_raw, modality="RTDOSE", rows=12, cols=12, frames=6, bits=32, position=(-14.2, -13.1, 7.3),
                   spacing=(2.5, 2.5), thickness=4.0, frame_uid="1.9.9")
    ct = host.VolumeFile.from_dicom(str(ctd))
    rt = host.VolumeFile.from_dicom(str(dsd))
    assert ct.GetSize() == (n, n, nz) and rt.GetSize() == (12, 12, 6)
    dose = np.array(rt.data(), f32)  # (as read: no scene has prepared the file)
    assert float(dose[..., 3].max()) > 1000.0
    dose[..., 3] = dose[..., 3] / f32(max(float(dose[..., 3].max()), 1.0))  # (a dose in [0, 1], whatever the file's scaling)
    shape = (nz, n, n)
    z, y, x = np.meshgrid(np.arange(nz), np.arange(n), np.arange(n), indexing="ij")
    ball = (x - 19.0) ** 2 + (y - 18.0) ** 2 + ((z - 5.5) * 2.5) ** 2 <= 11.0 ** 2
    mask = np.zeros(shape + (4,), f32)
    mask[..., 1] = ball
    bins, scale = 50, 50.0

    def grid_of(f):
        p = f.dicom_params()
        return f.GetSize(), tuple(p["ImagePositionPatient"]), (p["PixelSpacing"][0], p["PixelSpacing"][1], p["SliceThickness"])

    with host.Application(W, H, 0) as app:
        app.OnStart(capi.BASIC, [ct])
        c = app.context()
        c.volume_upload(0, dose)  # (in place of the scene's CT)
        c.volume_upload(1, mask)
        with pytest.raises(capi.VrError) as e:  # the gap: the dose lies on another grid than the mask
            app.dose_volume_histogram(0, 1, 1, bins, scale)
        assert e.value.code == capi.VR_ERR_INVALID_ARG
        res = app.resample_onto(rt, 0, ct, 2, channels=8, filter=capi.RESAMPLE_LINEAR, outside=(0, 0, 0, 0))
        got = c.volume_download(2, shape)
        geom = rr.between(*grid_of(rt), *grid_of(ct))
        want, want_res, box, copied = rr.resample(dose, None, (n, n, nz), 8, rr.LINEAR, *geom, (0, 0, 0, 0), (0, 0, 0), (n, n, nz))
        assert rr.same(got, want, copied) and res.as_tuple() == want_res and res.inside > 0 and res.outside > 0
        dvh = app.dose_volume_histogram(2, 1, 1, bins, scale)
        hd = capi.HistDesc()
        hd.volume_slot, hd.mask_slot, hd.channel, hd.bins, hd.scale, hd.out_of_range, hd.rows = 2, 1, 3, bins, scale, capi.HIST_CLAMP, 2 << 1
        hd = hd.copy(lo=(0, 0, 0), hi=(n, n, nz))
        counts, _, _ = hh.histogram(hd, want, mask)
        at_least = np.cumsum(counts[2][::-1])[::-1]
        assert np.array_equal(dvh, at_least.astype(np.uint64)) and int(dvh[0]) == int(ball.sum()) and 0 < int(dvh[bins // 4]) < int(dvh[0])
        # a caller's matrix: the identity written out gives the same slot; a shift by one CT voxel along x gives another
        eye = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]
        app.resample_onto(rt, 0, ct, 2, channels=8, dst_to_src=eye)
        assert np.array_equal(vt.bits(c.volume_download(2, shape)), vt.bits(got))
        shift = [1, 0, 0, 0.977, 0, 1, 0, 0, 0, 0, 1, 0]
        res = app.resample_onto(rt, 0, ct, 2, channels=8, dst_to_src=shift)
        geom = rr.between(*grid_of(rt), *grid_of(ct), shift)
        want, want_res, _, copied = rr.resample(dose, got, (n, n, nz), 8, rr.LINEAR, *geom, (0, 0, 0, 0), (0, 0, 0), (n, n, nz))
        assert rr.same(c.volume_download(2, shape), want, copied) and res.as_tuple() == want_res
        # the slot sizes must match the files
        with pytest.raises(capi.VrError) as e:
            app.resample_onto(ct, 0, ct, 2)
        assert e.value.code == capi.VR_ERR_INVALID_ARG
        with pytest.raises(capi.VrError) as e:
            app.resample_onto(rt, 0, rt, 2)
        assert e.value.code == capi.VR_ERR_INVALID_ARG
