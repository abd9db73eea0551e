"""GPU side of the slice views (vr_slice_async / vr_slice_render, csrc/vr_slice.h): images and counters bit-exact against the float32
restatement (slice_ref.py, pinned on the CPU by tests/test_slice.py) for every reduction, filter, format and arithmetic mode; the same
bits from every layout with skipping on and off; other volume and TF slots; hostile inputs; the stream order of table edits; no
interference with the viewport's renders; pick to slices; the host surface."""
import ctypes as C

import numpy as np
import pytest

import host_ref as hr
import proj_ref as pr
import slice_ref as sr
import vrtest as vt
from volumerendering_amd import capi

pytestmark = pytest.mark.gpu
f32 = np.float32
W, H = 64, 48    # the viewport: nothing a slice depends on
SW, SH = 40, 24  # the slices' output: no multiple of the 8 x 8 tile
REDUCE = [sr.MAX, sr.MIN, sr.AVERAGE]
FILTER = [sr.LINEAR, sr.NEAREST]


def noise(shape=(24, 20, 12), seed=5):
    nx, ny, nz = shape
    v = np.zeros((nz, ny, nx, 4), f32)
    v[..., 3] = np.random.default_rng(seed).integers(0, 4096, size=(nz, ny, nx)).astype(f32) / f32(4096.0)
    return v


def phantom():
    return vt.make_volume("phantom", 16)


def air_and_core(n=24):
    """Exact-zero air around a bright core: most bricks are inert for every reduction."""
    v = np.zeros((n, n, n, 4), f32)
    c = n // 2
    v[c - 3:c + 3, c - 3:c + 3, c - 3:c + 3, 3] = f32(0.9)
    v[c - 1:c + 1, c - 1:c + 1, c - 1:c + 1, 3] = f32(1.0)
    return v


def tf_pair(res=256):
    return hr.default_opacity_tf(res), hr.default_color_tf(res)


def desc(origin, du, dv, dn, steps, **over):
    d = capi.SliceDesc()
    d.volume_slot, d.tf_slot, d.width, d.height, d.slab_steps = 0, 0, SW, SH, steps
    return d.copy(origin=origin, du=du, dv=dv, dn=dn, **over)


def axial(nz, steps, **over):
    """The plane z = const through slab centre 0.4, stepping one voxel along z."""
    return desc((0.5 / SW, 0.5 / SH, 0.4), (1.0 / SW, 0, 0), (0, 1.0 / SH, 0), (0, 0, 1.0 / nz), steps, **over)


def oblique(steps, **over):
    """Tilted against all three axes; leaves the cube in one corner (pixels with n == 0)."""
    return desc((0.07, -0.05, 0.31), (0.9 / SW, 0.35 / SW, 0.2 / SW), (-0.2 / SH, 1.0 / SH, 0.45 / SH), (0.011, -0.013, 0.023), steps, **over)


def outside(steps, **over):
    return desc((1.5, 0.2, 0.2), (0.5 / SW, 0, 0), (0, 0.5 / SH, 0), (0.01, 0, 0), steps, **over)


def same(a, b):
    """Bit-equal, NaN where the other is NaN."""
    if a.dtype == np.uint8:
        return np.array_equal(a, b)
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    fin = ~np.isnan(b)
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(vt.bits(a)[fin], vt.bits(b)[fin])


def check(ctx, d, v, tf, fused=False, what=None):
    """The slice of the uploaded scene against the restatement, in both formats; returns the counters."""
    ref, n_ref, cov_ref = sr.slice_frame(d.copy(format=sr.RGBA32F), v, tf, fused)
    cnt = None
    for fmt in (sr.RGBA32F, sr.BGRA8):
        got = ctx.slice(d.copy(format=fmt))
        want = ref if fmt == sr.RGBA32F else sr.present(ref)
        assert got.shape == want.shape and got.dtype == want.dtype
        assert same(got, want), (what, fmt, fused)
        cnt = ctx.slice_counters()
        assert cnt[:2] == (n_ref, cov_ref), (what, fmt, cnt, n_ref, cov_ref)
        assert cnt[2] <= cnt[0]
    return cnt


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


@pytest.mark.parametrize("filt", FILTER)
@pytest.mark.parametrize("reduce", REDUCE)
def test_matches_restatement(ctx, reduce, filt):
    """Every reduction x filter x format in both arithmetic modes: 16^3 and 24 x 20 x 12 volumes, slabs of 1, 7 and 33 steps, an
    axis-aligned plane, an oblique one with uncovered pixels and one wholly outside, tables of 2 and 256 texels."""
    scenes = [
        (phantom(), tf_pair(2), [axial(16, 1), outside(7)]),
        (noise(), tf_pair(256), [oblique(7), oblique(33), axial(12, 1), axial(12, 33)]),
    ]
    for v, tf, planes in scenes:
        ctx.volume_upload(0, v)
        ctx.tf_upload(0, *tf)
        for fused in (False, True):
            ctx.set_arithmetic(capi.ARITH_FUSED if fused else capi.ARITH_SEPARATE)
            for k, d in enumerate(planes):
                cnt = check(ctx, d.copy(reduce=reduce, filter=filt), v, tf, fused, (v.shape, k))
                if d.origin[0] > 1.0:
                    assert cnt == (0, 0, 0)
    # the oblique plane really has both kinds of pixel
    _, n, _ = sr.reduce_slab(oblique(7), noise())
    assert 0 < int((n == 0).sum()) < n.size


@pytest.mark.parametrize("filt", FILTER)
@pytest.mark.parametrize("reduce", REDUCE)
def test_layouts_and_skipping(ctx, reduce, filt):
    """Layouts 0, 1, 3 x flavours 0, 1: identical images and out[0..1]; with skipping the phantom's empty bricks are not loaded
    (out[2] < out[0]), without it every counted sample is."""
    v, tf = air_and_core(), tf_pair(64)
    ctx.volume_upload(0, v)
    ctx.tf_upload(0, *tf)
    for d in (oblique(33, reduce=reduce, filter=filt), axial(24, 7, reduce=reduce, filter=filt)):
        ref, n_ref, cov_ref = sr.slice_frame(d, v, tf)
        assert n_ref > 0
        for layout in (0, 1, 3):
            ctx.set_volume_layout(layout)
            for fl in (0, 1):
                ctx.set_kernel_flavour(fl)
                got = ctx.slice(d)
                assert same(got, ref), (layout, fl)
                n, cov, fetched = ctx.slice_counters()
                assert (n, cov) == (n_ref, cov_ref)
                assert fetched == n if fl == 1 else fetched < n, (layout, fl, fetched, n)


def test_other_slots_and_reupload(ctx):
    """Slot 1 (another size than slot 0's) and slot 2 through TF slot 1; a volume re-upload rebuilds the range records, so the
    skipping slice follows the new data."""
    v0, v1, v2 = phantom(), noise(), vt.dose_volume()
    tf0, tf1 = tf_pair(64), ((hr.default_opacity_tf(128) * f32(0.5)).astype(f32), hr.default_color_tf(128)[::-1].copy())
    for i, v in enumerate((v0, v1, v2)):
        ctx.volume_upload(i, v)
    ctx.tf_upload(0, *tf0)
    ctx.tf_upload(1, *tf1)
    for reduce in REDUCE:
        check(ctx, oblique(7, volume_slot=1, tf_slot=1, reduce=reduce), v1, tf1, what="slot 1")
        check(ctx, oblique(7, volume_slot=2, tf_slot=1, reduce=reduce, filter=sr.NEAREST), v2, tf1, what="slot 2")
        check(ctx, oblique(7, volume_slot=0, tf_slot=0, reduce=reduce), v0, tf0, what="slot 0")
    new = air_and_core()
    ctx.volume_upload(1, new)
    for reduce in REDUCE:
        cnt = check(ctx, oblique(33, volume_slot=1, tf_slot=1, reduce=reduce), new, tf1, what="re-upload")
        assert cnt[2] < cnt[0]


def test_hostile_inputs(ctx):
    """NaN and infinite plane vectors, NaN and infinite voxels, an all-zero volume under AVERAGE, and 65536 steps of a slab that
    leaves the cube after a few: each matches the restatement, none raises."""
    tf = tf_pair(64)
    ctx.tf_upload(0, *tf)
    v = noise()
    ctx.volume_upload(0, v)
    nan, inf = float("nan"), float("inf")
    for reduce in REDUCE:
        for filt in FILTER:
            kw = dict(reduce=reduce, filter=filt)
            check(ctx, oblique(7, **kw).copy(du=(nan, 0.01, 0.0)), v, tf, what="NaN du")
            check(ctx, oblique(7, **kw).copy(du=(inf, 0.01, 0.0)), v, tf, what="inf du")
            check(ctx, oblique(7, **kw).copy(dn=(0.01, nan, 0.0)), v, tf, what="NaN dn")
            check(ctx, oblique(7, **kw).copy(dn=(0.01, -inf, 0.0)), v, tf, what="inf dn")
            cnt = check(ctx, oblique(65536, **kw).copy(dn=(0.21, 0.0, 0.05)), v, tf, what="65536 steps")
            assert 0 < cnt[0] <= 5 * SW * SH
    bad = noise(seed=6)
    bad[5, 9, 11, 3] = f32(nan)
    bad[7, 3, 20, 3] = f32(inf)
    bad[2, 15, 4, 3] = f32(-inf)
    ctx.volume_upload(0, bad)
    for reduce in REDUCE:
        for filt in FILTER:
            for fl in (0, 1):
                ctx.set_kernel_flavour(fl)
                check(ctx, oblique(33, reduce=reduce, filter=filt), bad, tf, what=("bad voxels", fl))
    ctx.set_kernel_flavour(0)
    zero = np.zeros((12, 20, 24, 4), f32)
    ctx.volume_upload(0, zero)
    cnt = check(ctx, oblique(33, reduce=sr.AVERAGE), zero, tf, what="zeros")
    assert cnt[0] > 0 and cnt[2] == 0


def test_validation_enqueues_nothing(ctx):
    v, tf = phantom(), tf_pair(64)
    ctx.volume_upload(0, v)
    ctx.tf_upload(0, *tf)
    good = oblique(7)
    ctx.slice(good)
    before = ctx.slice_counters()
    invalid = [dict(volume_slot=-1), dict(volume_slot=capi.MAX_VOLUMES), dict(tf_slot=-1), dict(tf_slot=2), dict(width=0), dict(height=0),
               dict(width=16385), dict(height=16385), dict(slab_steps=0), dict(slab_steps=65537), dict(reduce=3), dict(reduce=-1),
               dict(filter=2), dict(format=2)]
    out = np.zeros((SH, SW, 4), f32)
    for over in invalid:
        d = good.copy(**over)
        assert ctx.lib.vr_slice_render(ctx.h, C.byref(d), out.ctypes.data) == capi.VR_ERR_INVALID_ARG, over
        assert ctx.lib.vr_slice_async(ctx.h, C.byref(d), out.ctypes.data, None) == capi.VR_ERR_INVALID_ARG, over
    assert ctx.lib.vr_slice_render(ctx.h, None, out.ctypes.data) == capi.VR_ERR_INVALID_ARG
    assert ctx.lib.vr_slice_render(ctx.h, C.byref(good), None) == capi.VR_ERR_INVALID_ARG
    assert ctx.lib.vr_slice_async(ctx.h, C.byref(good), None, None) == capi.VR_ERR_INVALID_ARG
    assert ctx.lib.vr_slice_counters(ctx.h, None) == capi.VR_ERR_INVALID_ARG
    assert ctx.lib.vr_slice_orthogonal(ctx.h, 0, 3, 0, 1, C.byref(capi.SliceDesc())) == capi.VR_ERR_INVALID_ARG
    assert ctx.lib.vr_slice_orthogonal(ctx.h, 0, 0, 16, 1, C.byref(capi.SliceDesc())) == capi.VR_ERR_INVALID_ARG
    assert ctx.lib.vr_slice_orthogonal(ctx.h, 0, 0, 0, 0, C.byref(capi.SliceDesc())) == capi.VR_ERR_INVALID_ARG
    assert ctx.lib.vr_slice_orthogonal(ctx.h, 0, 0, 0, 1, None) == capi.VR_ERR_INVALID_ARG
    with capi.Context(W, H, 0) as empty:  # nothing uploaded: the slot, then its tables
        assert empty.lib.vr_slice_render(empty.h, C.byref(good), out.ctypes.data) == capi.VR_ERR_NOT_READY
        assert empty.lib.vr_slice_orthogonal(empty.h, 0, 0, 0, 1, C.byref(capi.SliceDesc())) == capi.VR_ERR_NOT_READY
        empty.volume_upload(0, v)
        assert empty.lib.vr_slice_render(empty.h, C.byref(good), out.ctypes.data) == capi.VR_ERR_NOT_READY
        assert empty.slice_counters() == (0, 0, 0)
    assert ctx.slice_counters() == before
    assert not out.any()


def test_orthogonal_descriptor(ctx):
    """vr_slice_orthogonal against its restatement, byte for byte: every axis, slabs that run past a face; and the slab's image."""
    v, tf = noise(), tf_pair(64)
    ctx.volume_upload(1, v)
    ctx.tf_upload(0, *tf)
    for axis, n in enumerate((24, 20, 12)):
        for index, thick in ((0, 1), (n - 1, 1), (n // 2, 4), (1, 7), (n - 1, 6)):
            d = ctx.slice_orthogonal(1, axis, index, thick)
            assert bytes(d) == bytes(sr.orthogonal_desc((24, 20, 12), axis, index, thick, slot=1)), (axis, index, thick)
            got = ctx.slice(d)
            ref, n_ref, cov_ref = sr.slice_frame(d, v, tf)
            assert same(got, ref) and ctx.slice_counters()[:2] == (n_ref, cov_ref)
            lo = index - (thick - 1) // 2
            assert n_ref == d.width * d.height * (min(lo + thick, n) - max(lo, 0)), (axis, index, thick)  # clipped, not moved


def test_stream_order_of_table_edits(ctx):
    """A slice enqueued on another stream after an asynchronous colour edit shows the new table, one enqueued before it the old one;
    nine slices in a row (one more than the launches in flight) come back."""
    v, tf = noise(), tf_pair(64)
    new_color = hr.default_color_tf(64)[::-1].copy()
    ctx.volume_upload(0, v)
    d = oblique(33)
    with capi.Context(SW, SH, 0) as a, capi.Context(SW, SH, 0) as b:
        for _ in range(3):  # (several rounds: the table's generations are reused behind their readers)
            ctx.tf_upload(0, *tf)
            ctx.slice_async(d, a.frame_device_ptr(), ctx.stream(1))
            ctx.tf_upload_async(0, color=new_color, stream=ctx.stream(0))
            ctx.slice_async(d, b.frame_device_ptr(), ctx.stream(2))
            for k in range(9):
                ctx.slice_async(d, b.frame_device_ptr(), ctx.stream(2 + k % 2))
            ctx.slice_counters()
            ctx.tf_upload(1, *tf)  # (a synchronous upload drains the device: every stream's slices have finished)
            old, _, _ = sr.slice_frame(d, v, tf)
            new, _, _ = sr.slice_frame(d, v, (tf[0], new_color))
            assert not same(old, new)
            assert same(a.download()[0], old)
            assert same(b.download()[0], new)


def test_no_interference_with_renders(ctx):
    """render, slice, download: the frame, counters, last flavour, kernel times and kernel choice are what the render left; a
    projection before and after slices of slot 0 gives the same frame and flavour; vr_resize between two slices changes nothing."""
    v, tf = vt.make_volume("phantom", 16, gradient=True), tf_pair(64)
    step, count = hr.stepping_params(16, 16, 16)
    u = hr.make_uniforms(W, H, steps_count=count, step_size=step)
    d = oblique(33)
    ref, _, _ = sr.slice_frame(d, v, tf)
    for variant in (capi.LIGHT, capi.MIP):
        ctx.reset_kernel_times()
        frag, _, _ = vt.gpu_render(ctx, variant, u, [v], [tf])

        def state():
            return ctx.counters(), ctx.last_kernel_flavour(), len(ctx.kernel_times()), ctx.kernel_choice(), ctx.last_timing()

        before = state()
        assert before[1] == 19 or variant != capi.MIP
        for reduce in REDUCE:
            assert same(ctx.slice(d.copy(reduce=reduce)), sr.slice_frame(d.copy(reduce=reduce), v, tf)[0])
        assert state() == before
        assert np.array_equal(vt.bits(ctx.download()[0]), vt.bits(frag))
        ctx.render(variant)  # (its counters are still pending when the slices come)
        ctx.slice(d)
        assert ctx.counters()[:2] == before[0][:2]  # (the default may try another form of the same bits: flavour and fetched may move)
        assert np.array_equal(vt.bits(ctx.download()[0]), vt.bits(frag))
    first = ctx.slice(d)
    ctx.resize(W + 8, H - 8)
    try:
        assert same(ctx.slice(d), first) and same(first, ref)
    finally:
        ctx.resize(W, H)


def test_pick_to_slices(ctx):
    """vr_pick, then the three orthogonal planes through voxel[]: the slice's pixel at that voxel is the TF of value[0][3] (a voxel
    centre: every lerp fraction is 0)."""
    v = vt.make_volume("phantom", 16, gradient=True)
    tf = (np.minimum(hr.default_opacity_tf(64) * f32(4.0), f32(1.0)).astype(f32), hr.default_color_tf(64))
    step, count = hr.stepping_params(16, 16, 16)
    u = hr.make_uniforms(W, H, steps_count=count, step_size=step)
    vt.gpu_render(ctx, capi.LIGHT, u, [v], [tf])
    p = ctx.pick(capi.LIGHT, W // 2, H // 2)
    assert p.hit == 1
    vox = [int(x) for x in p.voxel]
    value = f32(p.value[0][3])
    assert value == v[vox[2], vox[1], vox[0], 3]
    o, rgb = pr.tf_lookup(tf[0], tf[1], np.array([value], f32))
    want = np.zeros((1, 4), f32)
    pr._blend(rgb, o, want, np.array([True]))
    for axis in range(3):
        for filt in FILTER:
            img = ctx.slice(ctx.slice_orthogonal(0, axis, vox[axis], 1).copy(filter=filt))
            ua, va = (1 if axis == 0 else 0), (1 if axis == 2 else 2)
            assert np.array_equal(vt.bits(img[vox[va], vox[ua]]), vt.bits(want[0])), (axis, filt)


def test_host_surface_slices():
    """Application.slice_through_pick and Application.slice equal the C ABI's results on the application's own context."""
    from volumerendering_amd import host, synth
    with host.Application(W, H, 0) as app:
        vol = host.VolumeFile.from_raw(synth.ct_phantom_raw_fast(32))
        app.OnStart(capi.LIGHT, [vol])
        app.set_surface_threshold(0.05)
        app.OnUpdate()
        app.OnRender()
        p = app.pick(W // 2, H // 2)
        assert p.hit == 1
        c = app.context()
        vec4 = c.volume_download(0, (32, 32, 32))
        tf = (np.asarray(app.scene_opacity_tf(0).table(), f32), np.asarray(app.scene_color_tf(0).table(), f32).reshape(-1, 4))
        lit = 0
        for axis in range(3):
            for thick in (1, 5):
                d = c.slice_orthogonal(0, axis, int(p.voxel[axis]), thick)
                want = c.slice(d)
                got = app.slice_through_pick(p, axis, thick)
                assert got.shape == want.shape and np.array_equal(vt.bits(got), vt.bits(want))
                assert np.array_equal(vt.bits(app.slice(d)), vt.bits(want))
                assert same(want, sr.slice_frame(d, vec4, tf)[0]), (axis, thick)
                lit += int(want[..., 3].max() > 0)
        # (the picked voxel holds the surface point and may itself be air: a thin plane across the view direction can be empty; the
        # planes along it, through the centre pixel's ray, cut the body)
        assert lit >= 2
        bgra = app.slice(c.slice_orthogonal(0, 2, int(p.voxel[2]), 1).copy(format=capi.SLICE_BGRA8))
        assert bgra.dtype == np.uint8 and bgra.shape[2] == 4
