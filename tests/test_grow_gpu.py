"""GPU side of region growing (vr_segment_grow, csrc/vr_grow.h): the downloaded mask EQUAL, bit for bit, to the breadth-first
restatement (grow_ref.py, pinned on the CPU by tests/test_grow.py), and the result and the box's voxel count equal too -- percolating
noise with hostile values, a snake through every brick, adjacency across brick borders, no wrap inside a brick word, box walls, the
bounds, channels, layouts and both kernel forms, exact settling and stale records, the modes and what they preserve, the errors, the
freshness of everything downstream of the mask, and the host surface."""
import ctypes as C

import numpy as np
import pytest

import grow_cases as gc
import grow_ref as gr
import host_ref as hr
import test_histogram_gpu as thg
import vrtest as vt
from volumerendering_amd import capi

pytestmark = pytest.mark.gpu
f32 = np.float32
W, H = 64, 48
NAN, INF = float("nan"), float("inf")
SMALL, LARGE = gc.SMALL, gc.LARGE


def vol_a(a):
    """A volume whose .a is `a` (the other channels zero)."""
    v = np.zeros(a.shape + (4,), f32)
    v[..., 3] = a
    return v


def desc(shape, seeds, lo, hi, conn=capi.GROW_FACES, box=None, **over):
    d = capi.GrowDesc()
    d.volume_slot, d.channel, d.mask_slot, d.contour, d.connectivity, d.mode = 0, 3, 1, 0, conn, capi.GROW_REPLACE
    blo, bhi = box if box else gc.whole(shape)
    return d.copy(**{"lo": lo, "hi": hi, "box_lo": blo, "box_hi": bhi, "seeds": seeds, **over})


def seeds_of(d):
    return [tuple(int(c) for c in d.seeds[i]) for i in range(d.n_seeds)]


def check(ctx, d, v, before, what=None):
    """One grow against the restatement: the mask bit for bit, the result and out[0].  `before`: the mask slot's voxels before the call
    (None: an empty slot).  Returns (result, counters, the downloaded mask, R, Q)."""
    shape = v.shape[:3]
    res = ctx.segment_grow(d)
    cnt = ctx.grow_counters()
    got = ctx.volume_download(d.mask_slot, shape)
    want, voxels, (lo, hi), box, r, q = gr.grow(v[..., d.channel], before, d.contour, d.lo, d.hi, d.connectivity, d.mode,
                                                 tuple(d.box_lo), tuple(d.box_hi), seeds_of(d))
    bad = np.argwhere(vt.bits(got) != vt.bits(want))
    assert bad.size == 0, (what, len(bad), bad[:4])
    assert res.as_tuple() == (voxels, lo, hi), (what, res.as_tuple(), (voxels, lo, hi))
    assert res.rounds >= 1
    assert cnt[0] == box and cnt[1] + cnt[2] <= cnt[0], (what, cnt, box)
    return res, cnt, got, r, q


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


@pytest.mark.parametrize("conn", [capi.GROW_FACES, capi.GROW_ALL])
def test_noise_small_every_box_and_seed_count(ctx, conn):
    """(13, 18, 23), no side a multiple of 4, hostile values; every box of the histogram tests; 1, 3 and 64 seeds from Q plus two that
    are not in Q; both forms."""
    v, lo, hi = gc.noise_case(SMALL, conn)
    ctx.volume_upload(0, v)
    state = thg.contours(SMALL)
    ctx.volume_upload(1, state)
    for box in thg.BOXES:
        b = box if box else gc.whole(SMALL)
        q = gr.qualifies(v[..., 3], lo, hi, *b)
        for n_seeds in (1, 3, 64):
            seeds = gc.seeds_from(q, n_seeds, seed=n_seeds) if q.any() else []
            if box is None and n_seeds == 1:
                seeds = [gc.largest_component_seed(q, conn)[0]]
            seeds = (seeds + gc.seeds_from(q, 2, seed=5, want=False))[:64]
            for flavour in (0, 1):
                ctx.set_kernel_flavour(flavour)
                res, cnt, after, r, _ = check(ctx, desc(SMALL, seeds, lo, hi, conn, b), v, state, what=(box, n_seeds, flavour))
                if box is None:  # (not vacuous: something is reached, and not everything that qualifies)
                    assert 0 < int(r.sum()) < int(q.sum())
                    if n_seeds == 1:
                        assert int(r.sum()) > 100
            state = after


@pytest.mark.parametrize("conn", [capi.GROW_FACES, capi.GROW_ALL])
def test_noise_large_many_workgroups(ctx, conn):
    """(40, 52, 72): 2340 bricks, several workgroups, a long frontier; from the largest component."""
    v, lo, hi = gc.noise_case(LARGE, conn)
    q = gr.qualifies(v[..., 3], lo, hi, *gc.whole(LARGE))
    # a seed of a large component without labelling the whole volume: the component of the first of a few seeds that exceeds 1000 voxels
    seed = next(s for s in gc.seeds_from(q, 64, seed=3) if int(gr.region(q, [s], conn).sum()) > 1000)
    ctx.volume_upload(0, v)
    ctx.volume_upload(1, np.zeros(LARGE + (4,), f32))
    res, _, after, r, _ = check(ctx, desc(LARGE, [seed], lo, hi, conn), v, np.zeros(LARGE + (4,), f32))
    assert 1000 < res.voxels < int(q.sum()) and res.rounds > capi.GROW_BATCH
    ctx.set_kernel_flavour(1)
    res1, _, after1, _, _ = check(ctx, desc(LARGE, [seed], lo, hi, conn), v, after)
    assert res1.as_tuple() == res.as_tuple() and np.array_equal(vt.bits(after), vt.bits(after1))


def test_snake_through_every_brick(ctx):
    a, first, last, length = gc.snake(24)
    v = vol_a(a)
    ctx.volume_upload(0, v)
    ctx.volume_upload(1, np.zeros_like(v))
    state = np.zeros_like(v)
    for flavour in (0, 1):
        ctx.set_kernel_flavour(flavour)
        for conn in (capi.GROW_FACES, capi.GROW_ALL):
            res, _, state, r, _ = check(ctx, desc(a.shape, [first], 0.5, 1.5, conn), v, state, what=(flavour, conn))
            assert res.voxels == length and r[last[2], last[1], last[0]]
            assert res.rounds > 4 * capi.GROW_BATCH  # several batch-and-look cycles: the path crosses 6 bricks per row, 144 rows


@pytest.mark.parametrize("origin", [(4, 4, 4), (20, 16, 12)])
def test_adjacency_across_brick_borders(ctx, origin):
    """Two 2^3 cubes that meet only at a corner, only along an edge, and across a face, at a brick corner inside the volume and at the
    volume's last, partial bricks ((23, 18, 14): x 20 .. 22, y 16 .. 17, z 12 .. 13)."""
    shape = (14, 18, 23)
    ox, oy, oz = origin
    ctx.volume_upload(1, np.zeros(shape + (4,), f32))
    state = np.zeros(shape + (4,), f32)
    for shift, joined_by in (((0, 0, 0), {capi.GROW_ALL}), ((0, 0, -2), {capi.GROW_ALL}), ((0, -2, -2), {capi.GROW_FACES, capi.GROW_ALL})):
        a = np.zeros(shape, f32)
        a[oz - 2:oz, oy - 2:oy, ox - 2:ox] = 1.0  # ends at the brick corner
        sx, sy, sz = ox + shift[0], oy + shift[1], oz + shift[2]
        hi_x, hi_y, hi_z = min(sx + 2, shape[2]), min(sy + 2, shape[1]), min(sz + 2, shape[0])
        a[sz:hi_z, sy:hi_y, sx:hi_x] = 1.0
        second = int((a != 0).sum()) - 8
        assert second > 0
        v = vol_a(a)
        ctx.volume_upload(0, v)
        for conn in (capi.GROW_FACES, capi.GROW_ALL):
            for flavour in (0, 1):
                ctx.set_kernel_flavour(flavour)
                res, _, state, _, _ = check(ctx, desc(shape, [(ox - 2, oy - 2, oz - 2)], 0.5, 1.5, conn), v, state, what=(shift, conn, flavour))
                assert res.voxels == (8 + second if conn in joined_by else 8), (shift, conn, flavour)


def test_no_wrap_inside_a_brick_word(ctx):
    """Bits 3 and 4, 12 and 16 of a brick word are neighbours in the word and not in the volume."""
    shape = (8, 8, 8)
    ctx.volume_upload(1, np.zeros(shape + (4,), f32))
    state = np.zeros(shape + (4,), f32)
    for pair in (((3, 0, 0), (0, 1, 0)), ((0, 3, 0), (0, 0, 1)), ((3, 3, 0), (0, 0, 1)), ((0, 0, 0), (3, 3, 3))):
        for org in ((0, 0, 0), (4, 4, 4)):
            a = np.zeros(shape, f32)
            for x, y, z in pair:
                a[org[2] + z, org[1] + y, org[0] + x] = 1.0
            v = vol_a(a)
            ctx.volume_upload(0, v)
            seed = tuple(o + p for o, p in zip(org, pair[0]))
            for conn in (capi.GROW_FACES, capi.GROW_ALL):
                for flavour in (0, 1):
                    ctx.set_kernel_flavour(flavour)
                    res, _, state, _, _ = check(ctx, desc(shape, [seed], 0.5, 1.5, conn), v, state, what=(pair, org, conn, flavour))
                    assert res.voxels == 1


def test_box_walls_stop_the_region(ctx):
    shape = (12, 12, 16)
    a = np.ones(shape, f32)
    v = vol_a(a)
    ctx.volume_upload(0, v)
    ctx.volume_upload(1, np.zeros(shape + (4,), f32))
    state = np.zeros(shape + (4,), f32)
    for box in (((2, 3, 1), (13, 9, 11)), ((4, 4, 4), (8, 8, 8)), ((5, 0, 0), (6, 12, 12)), ((0, 0, 0), (16, 12, 12))):
        for conn in (capi.GROW_FACES, capi.GROW_ALL):
            for flavour in (0, 1):
                ctx.set_kernel_flavour(flavour)
                res, cnt, state, _, _ = check(ctx, desc(shape, [box[0]], 1.0, 1.0, conn, box), v, state, what=(box, conn, flavour))
                assert res.voxels == cnt[0] and (tuple(res.lo), tuple(res.hi)) == box
    # a seed inside the volume and outside the box adds nothing
    res, _, state, _, _ = check(ctx, desc(shape, [(0, 0, 0)], 1.0, 1.0, box=((4, 4, 4), (8, 8, 8))), v, state)
    assert res.voxels == 0 and tuple(res.lo) == tuple(res.hi) == (0, 0, 0)


def test_bounds_channels_layouts_and_forms(ctx):
    v = thg.noise(SMALL)
    v[2:6, 3:9, 4:12, 3] = f32(0.25)
    v[3, 4, 5, 3] = NAN
    whole = gc.whole(SMALL)
    state = np.zeros(SMALL + (4,), f32)
    for layout in (0, 1, 3):
        ctx.set_volume_layout(layout)
        ctx.volume_upload(0, v)
        ctx.volume_upload(1, state)
        for flavour in (0, 1):
            ctx.set_kernel_flavour(flavour)
            seeds = [(4, 3, 2), (11, 8, 5), (0, 0, 0)]
            for lo, hi in ((0.75, 0.25), (NAN, 1.0), (0.0, NAN), (NAN, NAN)):
                res, _, state, _, _ = check(ctx, desc(SMALL, seeds, lo, hi), v, state, what=(layout, flavour, lo, hi))
                assert res.voxels == 0
            # every number qualifies, NaN does not: everything but the NaN voxels, which cut nothing off here
            res, _, state, r, q = check(ctx, desc(SMALL, seeds, -INF, INF, capi.GROW_ALL), v, state, what=(layout, flavour, "inf"))
            assert res.voxels == int((~np.isnan(v[..., 3])).sum())
            res, _, state, _, _ = check(ctx, desc(SMALL, seeds, 0.25, 0.25), v, state, what=(layout, flavour, "plateau"))
            assert res.voxels >= 4 * 6 * 8 - 1
            for channel in range(3):
                a = v[..., channel]
                fin = a[np.isfinite(a)]
                lo, hi = float(np.quantile(fin, 0.2)), float(np.quantile(fin, 0.8))
                q = gr.qualifies(a, lo, hi, *whole)
                res, cnt, state, _, _ = check(ctx, desc(SMALL, gc.seeds_from(q, 3, seed=channel), lo, hi, channel=channel, contour=channel + 1), v, state,
                                              what=(layout, flavour, channel))
                assert res.voxels > 0 and cnt[2] == 0 and cnt[1] == cnt[0]  # (no settling off channel 3)


def test_settling_counters_and_stale_records(ctx):
    """Air and core: the default form classifies whole bricks from the range records, flavour 1 loads everything; the masks agree; the
    same after vr_volume_normalize changed the values in place."""
    v = thg.air_and_core(24)
    n = 24 ** 3
    ctx.volume_upload(0, v)
    ctx.volume_upload(1, np.zeros_like(v))
    state = np.zeros_like(v)
    c = 12
    for lo, hi, seed in ((0.5, INF, (c, c, c)), (-INF, INF, (0, 0, 0)), (0.5, 3.0e38, (c, c, c))):
        ctx.set_kernel_flavour(0)
        res, cnt, state, _, _ = check(ctx, desc(v.shape, [seed], lo, hi), v, state, what=(lo, hi))
        assert cnt[2] > 0 and cnt[2] % 64 == 0 and cnt[1] + cnt[2] == cnt[0] == n
        ctx.set_kernel_flavour(1)
        res1, cnt1, state1, _, _ = check(ctx, desc(v.shape, [seed], lo, hi), v, state, what=(lo, hi, "plain"))
        assert cnt1 == (n, n, 0) and res1.as_tuple() == res.as_tuple() and np.array_equal(vt.bits(state), vt.bits(state1))
        assert res.voxels == (n if lo < 0 else 6 ** 3)
    # a box that cuts bricks: only whole units inside it settle
    ctx.set_kernel_flavour(0)
    _, cnt, state, _, _ = check(ctx, desc(v.shape, [(c, c, c)], 0.5, INF, box=((1, 1, 1), (23, 23, 22))), v, state)
    assert 0 < cnt[2] <= 4 * 4 * 4 * 64 and cnt[1] + cnt[2] == cnt[0]
    # stale records: the values change in place, the grow classifies by the new ones
    raw = np.zeros((24, 24, 24), np.uint16)
    raw[8:16, 8:16, 8:16] = 700
    raw[0:4, 0:4, 0:4] = 1000
    ctx.volume_upload_raw(0, raw)
    before = ctx.volume_download(0, raw.shape)
    res, cnt, state, _, _ = check(ctx, desc(raw.shape, [(12, 12, 12)], 600.0, 800.0), before, state)
    assert res.voxels == 512 and cnt[2] > 0
    ctx.volume_normalize(0)
    after = ctx.volume_download(0, raw.shape)
    assert not np.array_equal(before[..., 3], after[..., 3])
    res, cnt, state, _, _ = check(ctx, desc(raw.shape, [(12, 12, 12)], 600.0, 800.0), after, state)
    assert res.voxels == 0 and cnt[2] > 0 and cnt[1] + cnt[2] == cnt[0]
    res, cnt, state, _, _ = check(ctx, desc(raw.shape, [(12, 12, 12)], 0.6, 0.8), after, state)
    assert res.voxels == 512 and cnt[2] > 0


def test_modes_preserve_everything_else_and_slots_are_created(ctx):
    v, lo, hi = gc.noise_case(SMALL, capi.GROW_FACES)
    q = gr.qualifies(v[..., 3], lo, hi, *gc.whole(SMALL))
    seeds = [gc.largest_component_seed(q, capi.GROW_FACES)[0]]
    m = thg.contours(SMALL)  # components holding NaN, negative and tiny values and -0
    for contour in range(4):
        for flavour in (0, 1):
            ctx.set_kernel_flavour(flavour)
            ctx.volume_upload(0, v)
            ctx.volume_upload(1, m)
            _, _, after, r, _ = check(ctx, desc(SMALL, seeds, lo, hi, mode=capi.GROW_ADD, contour=contour), v, m, what=("add", contour))
            keep = [c for c in range(4) if c != contour]
            assert np.array_equal(vt.bits(after[..., keep]), vt.bits(m[..., keep]))
            assert np.array_equal(vt.bits(after[..., contour][~r]), vt.bits(m[..., contour][~r])) and (after[..., contour][r] == 1.0).all()
            # REPLACE inside a small box clears the contour outside the box too
            box = ((4, 4, 4), (12, 12, 10))
            qb = gr.qualifies(v[..., 3], lo, hi, *box)
            _, _, rep, rb, _ = check(ctx, desc(SMALL, gc.seeds_from(qb, 5, seed=1), lo, hi, box=box, contour=contour), v, after, what=("replace", contour))
            assert rb.any() and not vt.bits(rep[..., contour][~rb]).any()
            assert np.array_equal(vt.bits(rep[..., keep]), vt.bits(m[..., keep]))
    # an empty mask slot is created with the value volume's dimensions, all +0
    for mode in (capi.GROW_REPLACE, capi.GROW_ADD):
        for flavour in (0, 1):
            with capi.Context(W, H, 0) as fresh:
                fresh.set_kernel_flavour(flavour)
                fresh.volume_upload(0, v)
                d = desc(SMALL, seeds, lo, hi, mode=mode, mask_slot=2, contour=2)
                res, _, made, _, _ = check(fresh, d, v, None, what=("fresh", mode, flavour))
                assert res.voxels > 100
                check(fresh, d.copy(lo=0.5, hi=0.25), v, made)  # (now it holds a mask: REPLACE stores the zeros)
                counts, rows = fresh.histogram(thg.desc(SMALL, mask_slot=2, rows=0b01000, bins=4, scale=1.0))
                assert rows[3][0] == (0 if mode == capi.GROW_REPLACE else res.voxels)


def test_errors_leave_the_mask_untouched(ctx):
    v = thg.noise(SMALL)
    m = thg.contours(SMALL)
    ctx.volume_upload(0, v)
    ctx.volume_upload(1, m)
    ctx.volume_upload(2, np.zeros((4, 4, 4, 4), f32))
    good = desc(SMALL, [(1, 1, 1)], 0.0, 0.5)
    ctx.segment_grow(good)
    m = ctx.volume_download(1, SMALL)
    counters = ctx.grow_counters()
    invalid = [dict(volume_slot=-1), dict(volume_slot=3), dict(mask_slot=-1), dict(mask_slot=3), dict(mask_slot=0), dict(channel=-1), dict(channel=4),
               dict(contour=-1), dict(contour=4), dict(connectivity=0), dict(connectivity=18), dict(mode=2), dict(mode=-1),
               dict(box_lo=(-1, 0, 0)), dict(box_hi=(24, 18, 13)), dict(box_hi=(23, 18, 14)), dict(box_lo=(5, 0, 0), box_hi=(4, 18, 13)),
               dict(n_seeds=0), dict(n_seeds=65), dict(seeds=[(23, 0, 0)]), dict(seeds=[(0, 0, 0), (0, -1, 0)]), dict(seeds=[(0, 0, 13)]),
               dict(mask_slot=2), dict(volume_slot=2, mask_slot=1)]
    for over in invalid:
        d = good.copy(**over)
        assert ctx.lib.vr_segment_grow(ctx.h, C.byref(d), C.byref(capi.GrowResult())) == capi.VR_ERR_INVALID_ARG, over
        assert (ctx.lib.vr_last_error(ctx.h) or b"").decode().startswith("vr_segment_grow"), over
    assert ctx.lib.vr_segment_grow(ctx.h, None, None) == capi.VR_ERR_INVALID_ARG
    assert ctx.lib.vr_segment_grow(None, C.byref(good), None) == capi.VR_ERR_INVALID_ARG
    assert ctx.lib.vr_grow_counters(ctx.h, None) == capi.VR_ERR_INVALID_ARG
    assert ctx.grow_counters() == counters
    assert np.array_equal(vt.bits(ctx.volume_download(1, SMALL)), vt.bits(m))
    assert np.array_equal(vt.bits(ctx.volume_download(2, (4, 4, 4))), np.zeros((4, 4, 4, 4), np.uint32))
    with capi.Context(W, H, 0) as empty:
        assert empty.grow_counters() == (0, 0, 0)
        assert empty.lib.vr_segment_grow(empty.h, C.byref(good), None) == capi.VR_ERR_NOT_READY
        assert b"empty" in empty.lib.vr_last_error(empty.h)
        assert empty.lib.vr_grow_whole(empty.h, 0, 1, 0, 0.0, 1.0, C.byref(capi.GrowDesc())) == capi.VR_ERR_NOT_READY
        with pytest.raises(capi.VrError):  # the mask slot was not created by the failed call
            empty.volume_download(1, SMALL)
    # vr_grow_whole
    d = ctx.grow_whole(0, 1, 2, -1.5, 2.5)
    assert bytes(d) == bytes(desc(SMALL, [], -1.5, 2.5, contour=2))
    for bad in ((3, 1, 0), (-1, 1, 0), (0, 3, 0), (0, -1, 0), (0, 0, 0), (0, 1, 4), (0, 1, -1)):
        assert ctx.lib.vr_grow_whole(ctx.h, *bad, 0.0, 1.0, C.byref(capi.GrowDesc())) == capi.VR_ERR_INVALID_ARG
    assert ctx.lib.vr_grow_whole(ctx.h, 0, 1, 0, 0.0, 1.0, None) == capi.VR_ERR_INVALID_ARG
    # a NULL result is fine
    assert ctx.lib.vr_segment_grow(ctx.h, C.byref(good), None) == capi.VR_OK


@pytest.mark.parametrize("variant", [capi.TF_CALIB, capi.VOLUME_MASK])
def test_everything_downstream_of_the_mask_is_fresh(variant):
    """After a grow into the mask slot of a scene, a render equals the render of a fresh context into which the downloaded mask was
    uploaded; the contour's histogram row sums to the result's voxels; the counters of the launches before the grow stay."""
    n = 16
    vols, tfs = vt.scene(variant, n)
    value_slot, mask_slot = (0, 1) if variant == capi.TF_CALIB else (2, 0)
    assert vols[mask_slot].shape == vols[value_slot].shape
    step, count = hr.stepping_params(n, n, n)
    u = hr.make_uniforms(W, H, steps_count=count, step_size=step)
    a = vols[value_slot][..., 3]
    z, y, x = (int(t) for t in np.unravel_index(int(np.argmax(a)), a.shape))
    lo = float(a[z, y, x]) * 0.5
    contour = 0  # (the component both shaders read)
    with capi.Context(W, H, 0) as ctx:
        before_frame, _, _ = vt.gpu_render(ctx, variant, u, vols, tfs)
        img = ctx.slice(ctx.slice_orthogonal(value_slot, 2, n // 2, 3))
        ctx.histogram(thg.desc(a.shape, volume_slot=value_slot, bins=64, scale=64.0))
        reports = ctx.counters(), ctx.last_kernel_flavour(), ctx.slice_counters(), ctx.hist_counters(), len(ctx.kernel_times())
        d = ctx.grow_whole(value_slot, mask_slot, contour, lo, INF).copy(seeds=[(x, y, z)], connectivity=capi.GROW_ALL)
        res, _, mask, r, _ = check(ctx, d, vols[value_slot], vols[mask_slot])
        assert res.voxels > 8
        assert (ctx.counters(), ctx.last_kernel_flavour(), ctx.slice_counters(), ctx.hist_counters(), len(ctx.kernel_times())) == reports
        assert np.array_equal(vt.bits(ctx.download()[0]), vt.bits(before_frame))
        assert np.array_equal(vt.bits(ctx.slice(ctx.slice_orthogonal(value_slot, 2, n // 2, 3))), vt.bits(img))
        ctx.render(variant)
        frame = ctx.download()[0]
        counts, rows = ctx.histogram(thg.desc(a.shape, volume_slot=value_slot, mask_slot=mask_slot, rows=2 << contour, bins=16, scale=1.0))
        assert rows[1 + contour][0] == res.voxels == int(counts[1 + contour].sum())
    fresh_vols = list(vols)
    fresh_vols[mask_slot] = mask
    with capi.Context(W, H, 0) as other:
        want, _, _ = vt.gpu_render(other, variant, u, fresh_vols, tfs)
    assert np.array_equal(vt.bits(frame), vt.bits(want))
    assert not np.array_equal(vt.bits(frame), vt.bits(before_frame))  # (the contour shows)


def test_application_grow_from_pick():
    from volumerendering_amd import host, synth
    with host.Application(W, H, 0) as app:
        app.OnStart(capi.LIGHT, [host.VolumeFile.from_raw(synth.ct_phantom_raw_fast(32))])
        app.set_surface_threshold(0.05)
        app.OnUpdate()
        app.OnRender()
        c = app.context()
        v = c.volume_download(0, (32, 32, 32))
        p = app.pick(W // 2, H // 2)
        assert p.hit == 1
        vox = tuple(int(t) for t in p.voxel)
        value = float(v[vox[2], vox[1], vox[0], 3])
        lo, hi = value - 0.125, value + 0.125
        for conn in (capi.GROW_FACES, capi.GROW_ALL):
            res = app.grow_from_pick(p, 0, 1, 2, lo, hi, conn)
            got = c.volume_download(1, (32, 32, 32))
            d = c.grow_whole(0, 2, 2, lo, hi).copy(seeds=[vox], connectivity=conn)
            want = c.segment_grow(d)
            assert res.as_tuple() == want.as_tuple() and res.voxels > 1
            assert np.array_equal(vt.bits(got), vt.bits(c.volume_download(2, (32, 32, 32))))
            ref = gr.grow(v[..., 3], None, 2, lo, hi, conn, gr.REPLACE, *gc.whole((32, 32, 32)), [vox])
            assert np.array_equal(vt.bits(got), vt.bits(ref[0])) and res.as_tuple() == (ref[1], *ref[2])
        miss = app.pick(0, 0)
        assert miss.hit == 0
        with pytest.raises(capi.VrError) as e:
            app.grow_from_pick(miss, 0, 1, 2, lo, hi)
        assert e.value.code == capi.VR_ERR_INVALID_ARG
