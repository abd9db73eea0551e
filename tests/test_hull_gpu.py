"""The hull of the active bricks on the device: the planes the distance-field build reduces (vr_skip_hull) against the numpy
restatement (tests/hull_ref.py), and frames of the skipping kernels, which prune their rays with it, against the forms that
skip nothing -- bit for bit, counters included."""
import numpy as np
import pytest

import hull_ref
import host_ref as hr
import vrtest as vt
from volumerendering_amd import capi

pytestmark = pytest.mark.gpu
f32 = np.float32


def prefix_tf(res, zeros, top=0.6):
    o = np.zeros(res, dtype=f32)
    o[zeros:] = np.linspace(0.0, top, res - zeros + 1, dtype=f32)[1:]
    return o, hr.default_color_tf(res)


# ---- planes ------------------------------------------------------------------------------------------------------------------------

NX, NY, NZ = 96, 64, 80  # three different sides: 24 x 16 x 20 bricks


def dense_volume(kind):
    z, y, x = np.meshgrid(np.arange(NZ), np.arange(NY), np.arange(NX), indexing="ij")
    if kind == "ellipsoid":  # its long axis along the (1, 1, 1) diagonal of the unit cube
        c = np.stack([x / NX - 0.5, y / NY - 0.5, z / NZ - 0.5], -1)
        d = np.array([1.0, 1.0, 1.0]) / np.sqrt(3.0)
        along = c @ d
        across = np.linalg.norm(c - along[..., None] * d, axis=-1)
        dense = (along / 0.62) ** 2 + (across / 0.16) ** 2 <= 1.0
    elif kind == "corner_brick":
        dense = (x == NX - 2) & (y == 1) & (z == NZ - 2)
    elif kind == "oblique_slab":
        dense = np.abs(x / NX + y / NY - z / NZ - 0.4) < 0.02
    elif kind == "nothing":
        dense = np.zeros((NZ, NY, NX), dtype=bool)
    elif kind == "everything":
        dense = np.ones((NZ, NY, NX), dtype=bool)
    else:
        raise ValueError(kind)
    v = np.zeros((NZ, NY, NX, 4), dtype=f32)
    v[..., 3] = dense
    return v


@pytest.mark.parametrize("kind", ["ellipsoid", "corner_brick", "oblique_slab", "nothing", "everything"])
def test_planes_are_the_restatements(kind):
    with capi.Context(64, 64, 0) as ctx:
        ctx.volume_upload(0, dense_volume(kind))
        ctx.tf_upload(0, *prefix_tf(64, 9))
        field, box, active = ctx.skip_field(capi.BASIC)
        assert field.shape == (NZ // 4, NY // 4, NX // 4)
        lo, hi = ctx.skip_hull(capi.BASIC)
        assert (lo, hi) == hull_ref.planes_of_field(field), kind
        if kind == "nothing":
            assert active == 0 and lo == (hull_ref.INT_MAX,) * 13 and hi == (hull_ref.INT_MIN,) * 13
        else:
            assert active == int((field == 0).sum()) > 0
            assert lo[:3] == box[:3] and hi[:3] == box[3:]
        if kind == "everything":
            assert lo[:3] == (0, 0, 0) and hi[:3] == (23, 15, 19) and lo[12] == -(15 + 19) and hi[9] == 23 + 15 + 19
        if kind == "corner_brick":
            assert active == 1 and lo == hi
        # a second build of the same context (another table) starts from zeroed words again
        ctx.tf_upload(0, *prefix_tf(64, 30))
        field2, _, _ = ctx.skip_field(capi.BASIC)
        assert ctx.skip_hull(capi.BASIC) == hull_ref.planes_of_field(field2)


# ---- frames ------------------------------------------------------------------------------------------------------------------------

N, W, H = 48, 128, 96
SKIPPING, PLAIN = (17, 6, 0), (1, 16)


def turn(n_cameras=12):
    step, count = hr.stepping_params(N, N, N)
    return [hr.make_uniforms(W, H, steps_count=count, step_size=step, distance=1.0 + 0.03 * k, yaw=2.0 * np.pi * k / n_cameras + 0.1,
                             pitch=0.35 - 0.06 * k) for k in range(n_cameras)]


def load_scene(ctx, variant):
    vols, tfs = vt.scene(variant, n=N)
    tfs = [prefix_tf(64, 9)] + list(tfs[1:])
    for i, v in enumerate(vols):
        ctx.volume_upload(i, v)
    for i, t in enumerate(tfs):
        ctx.tf_upload(i, t[0], t[1])


@pytest.fixture(scope="module")
def plain_frames():
    """Per variant: the turn's frames and counters rendered by the forms that skip nothing, computed once."""
    memo = {}

    def get(variant):
        if variant not in memo:
            out = {}
            with capi.Context(W, H, 0) as ctx:
                load_scene(ctx, variant)
                for fl in PLAIN:
                    ctx.set_kernel_flavour(fl)
                    rows = []
                    for u in turn():
                        ctx.set_uniforms(vt.to_capi_uniforms(u))
                        ctx.render(variant)
                        rows.append((ctx.download()[0], ctx.counters(), ctx.last_kernel_flavour()))
                    out[fl] = rows
            memo[variant] = out
        return memo[variant]
    return get


@pytest.mark.parametrize("per_launch", [1, 4])
@pytest.mark.parametrize("variant", [capi.LIGHT, capi.BASIC, capi.VOLUME_MASK])
def test_pruned_frames_are_the_plain_frames(variant, per_launch, plain_frames):
    ref = plain_frames(variant)
    us = turn()
    for k in range(len(us)):  # the two plain forms agree with each other (VOLUME_MASK has one: 16 runs as 17 there)
        assert np.array_equal(vt.bits(ref[1][k][0]), vt.bits(ref[16][k][0])) and ref[1][k][1][:2] == ref[16][k][1][:2]
        assert ref[1][k][2] == 1 and ref[1][k][1][2] == ref[1][k][1][0]  # (no skipping: every composited sample is fetched)
    fetched = {}
    outs = [capi.Context(W, H, 0) for _ in range(4)]
    try:
        with capi.Context(W, H, 0) as ctx:
            load_scene(ctx, variant)
            lo, hi = ctx.skip_hull(variant)
            assert hi[0] >= lo[0]  # (the scene has active bricks: there is a hull to prune with)
            for fl in SKIPPING:
                ctx.set_kernel_flavour(fl)
                for k0 in range(0, len(us), per_launch):
                    group = list(range(k0, k0 + per_launch))
                    if per_launch == 1:
                        ctx.set_uniforms(vt.to_capi_uniforms(us[k0]))
                        ctx.render_async(variant, outs[0].frame_device_ptr(), ctx.stream(0))
                    else:
                        ctx.render_batch_async(variant, [vt.to_capi_uniforms(us[k]) for k in group], [o.frame_device_ptr() for o in outs],
                                               ctx.stream(0))
                    counters = ctx.counters()  # (of the launch's last frame)
                    ran = ctx.last_kernel_flavour()
                    assert ran not in PLAIN, (fl, ran)
                    ctx.resize(W, H)  # drains the device
                    for j, k in enumerate(group):
                        got, _, _ = outs[j].download()
                        assert np.array_equal(vt.bits(got), vt.bits(ref[1][k][0])), (fl, k)
                    last = group[-1]
                    assert counters[:2] == ref[1][last][1][:2], (fl, last)
                    assert 0 < counters[2] < ref[1][last][1][2], (fl, last)
                    fetched.setdefault(last, {})[fl] = counters[2]
            assert ctx.unbounded_box_launches() == 0
    finally:
        for o in outs:
            o.close()
    # the hull prunes byte queries, never samples: what is fetched is the steps in active bricks, whichever kernel form walks them
    print("fetched per camera and flavour:", fetched)
    for k, by_flavour in fetched.items():
        assert len(set(by_flavour.values())) == 1, (k, by_flavour)


# ---- pending -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", [capi.LIGHT, capi.VOLUME_MASK])
def test_launches_behind_an_edit_run_without_a_hull(variant):
    """An asynchronous opacity edit rebuilds the field on its stream; until its planes have reached the host the launches get the
    unbounded hull and count as unbounded.  They render what a cold context renders with the hull in place -- the same frame and the
    same counters, `fetched` among them: pruning by the hull changes neither."""
    us = turn(4)
    tfs = [prefix_tf(128, 4 + 3 * k) for k in range(16)]
    vols, scene_tfs = vt.scene(variant, n=N)
    big = capi.Context(W, H * len(tfs), 0)
    cold = capi.Context(W, H, 0)
    try:
        with capi.Context(W, H, 0) as ctx:
            for c in (ctx, cold):
                c.set_kernel_flavour(17)
                load_scene(c, variant)
            ctx.set_uniforms(vt.to_capi_uniforms(us[0]))
            ctx.render(variant)
            miss0 = ctx.unbounded_box_launches()
            assert miss0 == 0
            st = [ctx.stream(k) for k in range(4)]
            base = big.frame_device_ptr()
            for k, tf in enumerate(tfs):
                ctx.tf_upload_async(0, opacity=tf[0], color=tf[1], stream=st[k & 3])
                ctx.set_uniforms(vt.to_capi_uniforms(us[k & 3]))
                ctx.render_async(variant, base + k * W * H * 16, st[k & 3])
            got_counters = ctx.counters()
            assert ctx.unbounded_box_launches() > miss0
            ctx.resize(W, H)
            frames, _, _ = big.download()
            for k, tf in enumerate(tfs):
                cold.tf_upload(0, tf[0], tf[1])
                cold.set_uniforms(vt.to_capi_uniforms(us[k & 3]))
                cold.render(variant)
                assert np.array_equal(vt.bits(frames[k * H:(k + 1) * H]), vt.bits(cold.download()[0])), k
            assert cold.unbounded_box_launches() == 0 and got_counters == cold.counters()
            # the planes of the last edit's field have arrived by now
            field, _, _ = ctx.skip_field(variant)
            assert ctx.skip_hull(variant) == hull_ref.planes_of_field(field) == cold.skip_hull(variant)
    finally:
        big.close()
        cold.close()
