"""GPU side of the device histograms (vr_histogram_async / vr_histogram, csrc/vr_hist.h): counts, row sums and the box's voxel count
EQUAL to the numpy restatement (hist_ref.py, pinned on the CPU by tests/test_histogram.py) for every path of the kernel -- the private
LDS copy and the global one, combining and exact settling against the plain form, partial brick units, masks and row sets, channels,
layouts -- plus the counters' promises, stale range records, stream order, isolation from the renders, the errors and the host surface."""
import ctypes as C

import numpy as np
import pytest

import hist_ref as hrf
import host_ref as hr
import vrtest as vt
from volumerendering_amd import capi

pytestmark = pytest.mark.gpu
f32 = np.float32
W, H = 64, 48
NAN, INF = float("nan"), float("inf")
SCALES = [256.0, 0.0, -3.5, 1e30, NAN]
POLICIES = [capi.HIST_CLAMP, capi.HIST_DROP]
SMALL = (13, 18, 23)  # nz, ny, nx: no side a multiple of 4
BOXES = [None, ((1, 2, 3), (22, 17, 12)), ((5, 7, 9), (6, 8, 10)), ((3, 3, 3), (3, 9, 9)), ((4, 8, 4), (8, 12, 8))]
# hostile values: NaN, infinities, negatives, -0, values in (-1 / scale, 0) for the scales above, huge ones
HOSTILE = np.array([NAN, INF, -INF, -0.3, -0.0, -0.001, -1e-3 / 256, 1e30, -1e30, 3.0e9, 0.999999, 1.0, 15.99], f32)


def noise(shape=SMALL, seed=11, hostile=True):
    """Every channel different; .a in [0, 1) on a 1/4096 grid with hostile voxels sprinkled in."""
    rng = np.random.default_rng(seed)
    v = (rng.integers(0, 4096, size=shape + (4,)).astype(f32) / f32(4096.0)).astype(f32)
    v[..., 0] *= f32(16.0)
    v[..., 1] -= f32(0.5)
    if hostile:
        k = rng.random(shape + (4,)) < 0.05
        v[k] = rng.choice(HOSTILE, size=int(k.sum()))
    return v


def contours(shape=SMALL, seed=12):
    """Four overlapping contours, the fourth empty; selected components carry NaN, negative and tiny values, unselected ones -0."""
    nz, ny, nx = shape
    rng = np.random.default_rng(seed)
    m = np.zeros(shape + (4,), f32)
    m[1:nz - 2, 2:ny - 3, 1:nx // 2, 0] = 1.0
    m[nz // 3:, ny // 4:, nx // 3:, 1] = rng.choice(np.array([1.0, NAN, -2.0, 1e-45, INF], f32), size=m[nz // 3:, ny // 4:, nx // 3:, 1].shape)
    m[..., 2] = np.where(rng.random(shape) < 0.1, f32(NAN), f32(-0.0))
    m[..., 3] = f32(-0.0)
    return m


def air_and_core(n=24):
    """Exact-zero air around a core (tests/test_slice_gpu.py's volume): most brick units settle."""
    v = np.zeros((n, n, n, 4), f32)
    c = n // 2
    v[c - 3:c + 3, c - 3:c + 3, c - 3:c + 3, 3] = f32(0.9)
    v[c - 1:c + 1, c - 1:c + 1, c - 1:c + 1, 3] = f32(1.0)
    return v


def desc(shape, box=None, **over):
    nz, ny, nx = shape[:3]
    d = capi.HistDesc()
    d.volume_slot, d.channel, d.mask_slot, d.rows, d.bins, d.scale, d.out_of_range = 0, 3, -1, 1, 256, 256.0, capi.HIST_CLAMP
    lo, hi = box if box else ((0, 0, 0), (nx, ny, nz))
    return d.copy(**{"lo": lo, "hi": hi, **over})


def check(ctx, d, v, m=None, what=None):
    """One histogram against the restatement: equality of counts, rows and out[0]; the sums; returns the counters."""
    counts, rows = ctx.histogram(d)
    cnt = ctx.hist_counters()
    want_counts, want_rows, box = hrf.histogram(d, v, m)
    assert counts.shape == want_counts.shape and counts.dtype == np.uint64
    assert np.array_equal(counts, want_counts), (what, np.argwhere(counts != want_counts)[:4])
    assert rows == want_rows, (what, rows, want_rows)
    assert cnt[0] == box, (what, cnt, box)
    assert cnt[1] + cnt[2] <= cnt[0]
    for r in range(hrf.ROWS):
        assert int(counts[r].sum()) + rows[r][1] == rows[r][0]
        if not (d.rows >> r) & 1:
            assert rows[r] == (0, 0) and not counts[r].any()
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


@pytest.fixture(scope="module")
def small():
    return noise(), contours()


@pytest.fixture(scope="module")
def large():
    """256 x 256 x 64: more brick units than the grid has wavefronts (a grid-stride walk), every workgroup flushes."""
    rng = np.random.default_rng(21)
    v = np.zeros((64, 256, 256, 4), f32)
    v[..., 3] = rng.random((64, 256, 256), dtype=f32)
    v[:24, :, :, 3] = 0.0       # air: settled units
    v[40:44, 100:104, 8:12, 3] = f32(0.5)
    return v


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("bins", [1, 7, 256, 4096])
def test_lds_path_matches_restatement(ctx, small, bins, policy):
    """The private LDS copy: every scale and box on the hostile 23 x 18 x 13 volume, unmasked (settling, density plane) and masked."""
    v, m = small
    ctx.volume_upload(0, v)
    ctx.volume_upload(1, m)
    for scale in SCALES:
        for box in BOXES:
            check(ctx, desc(SMALL, box, bins=bins, scale=scale, out_of_range=policy), v, what=(scale, box))
        check(ctx, desc(SMALL, BOXES[1], bins=bins, scale=scale, out_of_range=policy, mask_slot=1, rows=0b01111 if bins == 4096 else 0b11111), v, m,
              what=(scale, "masked"))


@pytest.mark.parametrize("policy", POLICIES)
def test_global_path_matches_restatement(ctx, small, policy):
    """Bin counts whose private copy exceeds the LDS budget add straight into global memory: 65 536 bins, and 40 000 x 5 rows."""
    v, m = small
    ctx.volume_upload(0, v)
    ctx.volume_upload(1, m)
    for scale in (65536.0, -3.5, NAN):
        for box in BOXES[:3]:
            check(ctx, desc(SMALL, box, bins=65536, scale=scale, out_of_range=policy), v, what=(scale, box))
        check(ctx, desc(SMALL, None, bins=40000, scale=scale * 0.5, out_of_range=policy, mask_slot=1, rows=0b11111), v, m)
    # either side of the budget (rows computed * bins <= 16384 words)
    for bins, rows in ((16384, 1), (16385, 1), (8192, 0b00011), (8193, 0b00011), (4096, 0b11111)):
        check(ctx, desc(SMALL, None, bins=bins, scale=float(bins), out_of_range=policy, mask_slot=1, rows=rows), v, m, what=(bins, rows))


@pytest.mark.parametrize("flavour", [0, 1])
def test_constant_volume_every_lane_one_bin(ctx, flavour):
    v = np.full((32, 32, 32, 4), f32(0.3), f32)
    ctx.volume_upload(0, v)
    ctx.set_kernel_flavour(flavour)
    for bins in (1, 256, 65536):
        for policy in POLICIES:
            for scale in (256.0, 1e30):
                d = desc(v.shape, bins=bins, scale=scale, out_of_range=policy)
                cnt = check(ctx, d, v)
                assert cnt == ((32768, 32768, 0) if flavour == 1 else (32768, 0, 32768))
                check(ctx, d.copy(lo=(1, 0, 0)), v)
                check(ctx, d.copy(channel=1), v)  # (no settling off channel 3: the combining alone)


def test_air_and_core_counters(ctx):
    """Unmasked channel 3: the default form settles air from the records and loads the rest; flavour 1 loads everything."""
    v = air_and_core(24)
    ctx.volume_upload(0, v)
    for bins, scale in ((256, 255.0), (4096, 4096.0), (65536, 3.0)):
        for policy in POLICIES:
            d = desc(v.shape, bins=bins, scale=scale, out_of_range=policy)
            ctx.set_kernel_flavour(0)
            cnt = check(ctx, d, v)
            assert cnt[2] > 0 and cnt[1] > 0 and cnt[1] + cnt[2] == cnt[0] == 24 ** 3
            assert cnt[2] % 64 == 0
            ctx.set_kernel_flavour(1)
            cnt = check(ctx, d, v)
            assert cnt[1] == cnt[0] and cnt[2] == 0
    # a box that cuts bricks: only whole units inside it may settle
    ctx.set_kernel_flavour(0)
    cnt = check(ctx, desc(v.shape, ((1, 1, 1), (23, 23, 22))), v)
    assert 0 < cnt[2] <= 4 * 4 * 4 * 64 and cnt[1] + cnt[2] == cnt[0]


@pytest.mark.parametrize("bins", [256, 4096, 65536])
def test_large_volume_many_blocks(ctx, large, bins):
    v = large
    ctx.volume_upload(0, v)
    want = None
    for flavour in (0, 1):
        ctx.set_kernel_flavour(flavour)
        d = desc(v.shape, bins=bins, scale=float(bins))
        counts, rows = ctx.histogram(d)
        cnt = ctx.hist_counters()
        if want is None:
            want = hrf.histogram(d, v)
        assert np.array_equal(counts, want[0]) and rows == want[1] and cnt[0] == want[2] == v.shape[0] * v.shape[1] * v.shape[2]
        assert int(counts[0].sum()) == rows[0][0] and rows[0][1] == 0
        if flavour == 0:
            assert cnt[2] >= 20 * 256 * 256 and cnt[1] + cnt[2] == cnt[0]
        else:
            assert cnt[1] == cnt[0] and cnt[2] == 0
    ctx.set_kernel_flavour(0)
    check(ctx, desc(v.shape, ((3, 5, 2), (250, 255, 61)), bins=bins, scale=float(bins) * 1.5, out_of_range=capi.HIST_DROP), v)


def test_every_row_set_and_slot_assignment(ctx, small):
    """Every legal value of `rows` with a mask (and rows = 1 without); value and mask slots exchanged."""
    v, m = small
    for vs, ms in ((0, 1), (2, 0)):
        ctx.volume_upload(vs, v)
        ctx.volume_upload(ms, m)
        for rows in range(1, 32):
            for flavour in (0, 1):
                ctx.set_kernel_flavour(flavour)
                check(ctx, desc(SMALL, BOXES[rows % 2], volume_slot=vs, mask_slot=ms, rows=rows, bins=64, scale=64.0, out_of_range=rows % 2), v, m,
                      what=(vs, ms, rows, flavour))
        ctx.set_kernel_flavour(0)
        check(ctx, desc(SMALL, volume_slot=vs, rows=1), v)
        # the mask volume's own values through the other slot as the mask: the roles are the descriptor's, not the slots'
        check(ctx, desc(SMALL, volume_slot=ms, mask_slot=vs, rows=0b10101, bins=7, scale=3.0, channel=1), m, v)


def test_every_channel(ctx, small):
    v, m = small
    ctx.volume_upload(0, v)
    ctx.volume_upload(1, m)
    results = []
    for channel in range(4):
        for policy in POLICIES:
            d = desc(SMALL, channel=channel, bins=300, scale=37.0, out_of_range=policy)
            check(ctx, d, v, what=channel)
            check(ctx, d.copy(mask_slot=1, rows=0b00110), v, m, what=channel)
        results.append(ctx.histogram(desc(SMALL, channel=channel, bins=300, scale=37.0))[0])
    assert all(not np.array_equal(results[3], results[c]) for c in range(3))


def test_forms_layouts_and_arithmetic_agree(ctx, small):
    """Flavour 1 and the default, layouts 0, 1 and 3 (with and without a density plane), both arithmetic modes: identical outputs."""
    v, m = small
    a = air_and_core(24)
    a[..., 0] = f32(7.0)
    for vol, mask in ((v, m), (a, None)):
        shape = vol.shape[:3]
        cases = [desc(shape, bins=256, scale=255.0), desc(shape, ((1, 2, 3), (11, 17, 12)), bins=4096, scale=-3.5, out_of_range=capi.HIST_DROP)]
        if mask is not None:
            cases.append(desc(shape, mask_slot=1, rows=0b10111, bins=97, scale=97.0))
        want = [hrf.histogram(d, vol, mask) for d in cases]
        for layout in (0, 1, 3):
            ctx.set_volume_layout(layout)
            ctx.volume_upload(0, vol)
            if mask is not None:
                ctx.volume_upload(1, mask)
            for arith in (capi.ARITH_SEPARATE, capi.ARITH_FUSED):
                ctx.set_arithmetic(arith)
                for flavour in (0, 1, 6):  # (6: any flavour but 1 is the default form)
                    ctx.set_kernel_flavour(flavour)
                    for d, (wc, wr, wb) in zip(cases, want):
                        counts, rows = ctx.histogram(d)
                        assert np.array_equal(counts, wc) and rows == wr and ctx.hist_counters()[0] == wb, (layout, arith, flavour)


def test_value_is_loaded_only_where_a_row_needs_it(ctx, small):
    v, _ = small
    m = np.zeros(SMALL + (4,), f32)
    m[2:5, 3:6, 4:9, 1] = 1.0
    m[3:6, 3:6, 6:11, 3] = NAN
    ctx.volume_upload(0, v)
    ctx.volume_upload(1, m)
    inside = int(((m[..., 1] != 0) | (m[..., 3] != 0)).sum())
    cnt = check(ctx, desc(SMALL, mask_slot=1, rows=0b10100), v, m)
    assert cnt[1] == inside < cnt[0] and cnt[2] == 0
    cnt = check(ctx, desc(SMALL, mask_slot=1, rows=0b00100), v, m)
    assert cnt[1] == int((m[..., 1] != 0).sum())
    cnt = check(ctx, desc(SMALL, mask_slot=1, rows=0b10101), v, m)
    assert cnt[1] == cnt[0]
    ctx.set_kernel_flavour(1)
    cnt = check(ctx, desc(SMALL, mask_slot=1, rows=0b10100), v, m)
    assert cnt[1] == inside and cnt[2] == 0


def test_stale_records_are_rebuilt(ctx):
    """A histogram, vr_volume_normalize in place, the histogram again: the second equals the restatement on the downloaded voxels."""
    raw = np.zeros((24, 24, 24), np.uint16)
    raw[8:16, 8:16, 8:16] = 700
    raw[10:14, 10:14, 10:14] = np.random.default_rng(5).integers(0, 1000, size=(4, 4, 4), dtype=np.uint16)
    raw[0:4, 0:4, 0:4] = 1000
    ctx.volume_upload_raw(0, raw)
    before = ctx.volume_download(0, raw.shape)
    d = desc(raw.shape, bins=1001, scale=1.0)
    cnt = check(ctx, d, before)
    assert cnt[2] > 0
    ctx.volume_normalize(0)
    after = ctx.volume_download(0, raw.shape)
    assert not np.array_equal(before[..., 3], after[..., 3])
    d2 = d.copy(scale=1000.0)
    cnt = check(ctx, d2, after)
    assert cnt[2] > 0 and cnt[1] + cnt[2] == cnt[0]
    assert not np.array_equal(ctx.histogram(d)[0], hrf.histogram(d, before)[0])  # (the old scale on the new voxels)
    check(ctx, d, after)


def test_two_async_launches_back_to_back(ctx, small):
    """Two vr_histogram_async calls on a caller's stream into different buffers, read after one synchronisation."""
    v, m = small
    ctx.volume_upload(0, v)
    ctx.volume_upload(1, m)
    bins = 256
    d1 = desc(SMALL, bins=bins, scale=255.0)
    d2 = desc(SMALL, BOXES[1], bins=bins, scale=31.0, mask_slot=1, rows=0b00111, out_of_range=capi.HIST_DROP)
    cbytes = hrf.ROWS * bins * 8
    assert cbytes + 80 <= W * H * 16
    with capi.Context(W, H, 0) as a, capi.Context(W, H, 0) as b:
        s = ctx.stream(1)
        for _ in range(5):  # (ten launches: more than may be in flight)
            ctx.histogram_async(d1, a.frame_device_ptr(), a.frame_device_ptr() + cbytes, s)
            ctx.histogram_async(d2, b.frame_device_ptr(), b.frame_device_ptr() + cbytes, s)
        cnt = ctx.hist_counters()  # waits for the last launch, and the stream runs them in order
        for c, d, mask in ((a, d1, None), (b, d2, m)):
            words = np.ascontiguousarray(c.download()[0]).view(np.uint64).ravel()
            wc, wr, wb = hrf.histogram(d, v, mask)
            assert np.array_equal(words[:hrf.ROWS * bins].reshape(hrf.ROWS, bins), wc)
            assert [tuple(int(x) for x in words[hrf.ROWS * bins + 2 * r:hrf.ROWS * bins + 2 * r + 2]) for r in range(hrf.ROWS)] == wr
        assert cnt[0] == hrf.histogram(d2, v, m)[2]


def test_no_interference_with_renders_and_slices(ctx):
    """render, histogram, download: the frame, vr_last_counters, the last flavour, the timings, the kernel choice and
    vr_slice_counters are what they were."""
    v, tf = vt.make_volume("phantom", 16, gradient=True), (hr.default_opacity_tf(64), hr.default_color_tf(64))
    step, count = hr.stepping_params(16, 16, 16)
    u = hr.make_uniforms(W, H, steps_count=count, step_size=step)
    ctx.reset_kernel_times()
    frag, _, _ = vt.gpu_render(ctx, capi.LIGHT, u, [v], [tf])
    sd = ctx.slice_orthogonal(0, 2, 8, 3)
    img = ctx.slice(sd)

    def state():
        return ctx.counters(), ctx.last_kernel_flavour(), len(ctx.kernel_times()), ctx.kernel_choice(), ctx.last_timing(), ctx.slice_counters()

    before = state()
    for flavour in (0, 1):
        ctx.set_kernel_flavour(flavour)
        check(ctx, desc(v.shape, bins=64, scale=64.0), v)
    ctx.set_kernel_flavour(0)
    assert state() == before
    assert np.array_equal(vt.bits(ctx.download()[0]), vt.bits(frag))
    ctx.render(capi.LIGHT)  # (its counters are still pending when the histogram comes)
    check(ctx, desc(v.shape, bins=64, scale=64.0), v)
    assert ctx.counters()[:2] == before[0][:2]
    assert np.array_equal(vt.bits(ctx.download()[0]), vt.bits(frag))
    assert np.array_equal(vt.bits(ctx.slice(sd)), vt.bits(img))


def test_hist_whole_descriptor(ctx, small):
    v, _ = small
    ctx.volume_upload(2, v)
    d = ctx.hist_whole(2, 77, -1.5)
    assert bytes(d) == bytes(desc(SMALL, volume_slot=2, bins=77, scale=-1.5))
    check(ctx, d, v)
    for bad in ((3, 16), (-1, 16), (2, 0), (2, 65537)):
        assert ctx.lib.vr_hist_whole(ctx.h, bad[0], bad[1], 1.0, C.byref(capi.HistDesc())) == capi.VR_ERR_INVALID_ARG
    assert ctx.lib.vr_hist_whole(ctx.h, 2, 16, 1.0, None) == capi.VR_ERR_INVALID_ARG
    assert ctx.hist_whole(2, 65536, NAN).bins == 65536


def test_errors_leave_outputs_untouched(ctx, small):
    v, m = small
    ctx.volume_upload(0, v)
    ctx.volume_upload(1, m)
    ctx.volume_upload(2, np.zeros((4, 4, 4, 4), f32))
    good = desc(SMALL, mask_slot=1, rows=0b00011, bins=16)
    ctx.histogram(good)
    before = ctx.hist_counters()
    counts = np.full((hrf.ROWS, 16), 7, np.uint64)
    rows = np.full(hrf.ROWS * 2, 9, np.uint64)
    invalid = [dict(volume_slot=-1), dict(volume_slot=3), dict(mask_slot=-2), dict(mask_slot=3), dict(channel=-1), dict(channel=4), dict(bins=0),
               dict(bins=65537), dict(out_of_range=2), dict(out_of_range=-1), dict(rows=0), dict(rows=32), dict(rows=0b100001),
               dict(mask_slot=-1), dict(mask_slot=-1, rows=0b00010), dict(lo=(-1, 0, 0)), dict(hi=(24, 18, 13)), dict(lo=(5, 0, 0), hi=(4, 18, 13)),
               dict(hi=(23, 18, 14)), dict(mask_slot=2)]
    for over in invalid:
        d = good.copy(**over)
        for rc in (ctx.lib.vr_histogram(ctx.h, C.byref(d), counts.ctypes.data, rows.ctypes.data),
                   ctx.lib.vr_histogram_async(ctx.h, C.byref(d), counts.ctypes.data, rows.ctypes.data, None)):
            assert rc == capi.VR_ERR_INVALID_ARG, over
            assert (ctx.lib.vr_last_error(ctx.h) or b"").decode().startswith("vr_histogram"), over
    for args in ((None, counts.ctypes.data, rows.ctypes.data), (C.byref(good), None, rows.ctypes.data), (C.byref(good), counts.ctypes.data, None)):
        assert ctx.lib.vr_histogram(ctx.h, *args) == capi.VR_ERR_INVALID_ARG
        assert ctx.lib.vr_histogram_async(ctx.h, *args, None) == capi.VR_ERR_INVALID_ARG
        assert b"NULL" in ctx.lib.vr_last_error(ctx.h)
    assert ctx.lib.vr_hist_counters(ctx.h, None) == capi.VR_ERR_INVALID_ARG
    with capi.Context(W, H, 0) as empty:
        assert empty.hist_counters() == (0, 0, 0)
        assert empty.lib.vr_histogram(empty.h, C.byref(good), counts.ctypes.data, rows.ctypes.data) == capi.VR_ERR_NOT_READY
        assert b"empty" in empty.lib.vr_last_error(empty.h)
        assert empty.lib.vr_hist_whole(empty.h, 0, 16, 1.0, C.byref(capi.HistDesc())) == capi.VR_ERR_NOT_READY
        empty.volume_upload(0, v)
        assert empty.lib.vr_histogram(empty.h, C.byref(good), counts.ctypes.data, rows.ctypes.data) == capi.VR_ERR_NOT_READY  # the mask slot
        assert empty.hist_counters() == (0, 0, 0)
    assert ctx.hist_counters() == before
    assert (counts == 7).all() and (rows == 9).all()
    # no value of scale is an error
    for scale in (NAN, INF, -INF, 0.0, 3.4e38):
        check(ctx, good.copy(scale=scale), v, m)


def test_device_activate_histogram_equals_cpu_overload(ctx):
    from volumerendering_amd import host
    raw = hr.ct_phantom_raw(16)
    for normalized in (False, True):
        vf = host.VolumeFile.from_raw(raw)
        if normalized:
            vf.NormalizeData()
        ctx.volume_upload(0, vf.data())
        for res in (256, 1000):
            tf = host.OpacityTF(res)
            cpu = tf.ActivateHistogram(vf).copy()
            dev = tf.ActivateHistogramDevice(ctx, 0, normalized, vf.GetDataRange())
            assert cpu.any() and np.array_equal(vt.bits(cpu), vt.bits(dev)), (normalized, res)


def test_device_calibrate_on_mask_equals_cpu_overload(ctx):
    """Channel 3 before normalisation, channel 0 after vr_volume_normalize (the raw value survives in .r)."""
    from volumerendering_amd import host
    n = 16
    raw = np.full((n, n, n), 100, dtype=np.uint16)
    raw[4:12, 4:12, 4:12] = 900
    raw[5:7, 5:7, 5:7] = 420
    raw[0, 0, 0] = 1000
    m = np.zeros((n, n, n, 4), dtype=f32)
    m[4:12, 4:12, 4:12, 0] = 1.0
    m[2:8, 2:8, 2:8, 2] = 1.0
    ct, mask = host.VolumeFile.from_raw(raw), host.VolumeFile.from_vec4(m, 1)
    for active in ((1, 0, 0, 0), (1, 0, 1, 0), (0, 0, 1, 1)):
        cpu = host.OpacityTF(1000)
        cpu.CalibrateOnMask(mask, ct, active)
        ctx.volume_upload_raw(0, raw)
        ctx.volume_upload(1, m)
        for channel in (3, 0):
            if channel == 0:
                ctx.volume_normalize(0)
            dev = host.OpacityTF(1000)
            dev.CalibrateOnMaskDevice(ctx, 0, 1, channel, ct.GetMaxNumber(), active)
            assert dev.GetControlPoints() == cpu.GetControlPoints(), (active, channel)
            assert np.array_equal(vt.bits(dev.table()), vt.bits(cpu.table())), (active, channel)
    assert len(cpu.GetControlPoints()) > 2


def test_dose_volume_histogram():
    """Application.dose_volume_histogram: the reversed cumulative sum of the contour's row; element 0 is its voxel count."""
    from volumerendering_amd import host, synth
    with host.Application(W, H, 0) as app:
        app.OnStart(capi.LIGHT, [host.VolumeFile.from_raw(synth.ct_phantom_raw_fast(32))])
        c = app.context()
        dose, m = noise((12, 20, 16), seed=31, hostile=False), contours((12, 20, 16), seed=32)
        c.volume_upload(1, dose)
        c.volume_upload(2, m)
        for contour in range(4):
            d = desc(dose.shape, volume_slot=1, mask_slot=2, rows=2 << contour, bins=50, scale=40.0)
            counts, rows, _ = hrf.histogram(d, dose, m)
            got = app.dose_volume_histogram(1, 2, contour, 50, 40.0)
            assert got.dtype == np.uint64 and np.array_equal(got, np.cumsum(counts[1 + contour][::-1])[::-1])
            assert int(got[0]) == rows[1 + contour][0] == int(hrf.selects(m[..., contour]).sum())
            ac, ar = app.histogram(d)
            assert np.array_equal(ac, counts) and ar == rows
        assert int(app.dose_volume_histogram(1, 2, 3, 50, 40.0)[0]) == 0  # the empty contour
