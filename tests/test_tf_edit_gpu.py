"""Stream-ordered transfer-function edits (vr_tf_upload_opacity_async / _color_async) and the separable distance-field builder
(vr_skip_field).  Every frame is compared bit for bit with a cold render: a second context that loads the same table with the
synchronous upload."""
import ctypes as C
import os
import time

import numpy as np
import pytest

import host_ref as hr
import vrtest as vt
from skip_ref import CAP, check_field, numpy_active  # (the numpy field, records and active bricks: tests/skip_ref.py)
from volumerendering_amd import capi

pytestmark = pytest.mark.gpu
f32 = np.float32


def prefix_tf(res, zeros, top=0.6):
    o = np.zeros(res, dtype=f32)
    o[zeros:] = np.linspace(0.0, top, res - zeros + 1, dtype=f32)[1:]
    return o, hr.default_color_tf(res)


def recolour(tf):
    c = tf[1].copy()
    c[:, 1] = f32(0.3)
    return tf[0], c


class Cold:
    """Reference renders: the same volumes in a context of their own, each table loaded with the synchronous upload."""

    def __init__(self, variant, vols, other_tfs, W, H, flavour):
        self.variant, self.other = variant, other_tfs
        self.ctx = capi.Context(W, H, 0)
        self.ctx.set_kernel_flavour(flavour)
        for i, v in enumerate(vols):
            self.ctx.volume_upload(i, v)
        self.memo = {}

    def __call__(self, tf, u, flavour=None):
        key = (tf[0].tobytes(), tf[1].tobytes(), bytes(vt.to_capi_uniforms(u)), flavour)
        if key not in self.memo:
            if flavour is not None:
                self.ctx.set_kernel_flavour(flavour)
            for i, t in enumerate([tf] + list(self.other)):
                self.ctx.tf_upload(i, t[0], t[1])
            self.ctx.set_uniforms(vt.to_capi_uniforms(u))
            self.ctx.render(self.variant)
            frag, _, _ = self.ctx.download()
            self.memo[key] = (frag, self.ctx.counters(), self.ctx.last_kernel_flavour())
        return self.memo[key]

    def close(self):
        self.ctx.close()


def setup(variant, n=24):
    if variant == capi.VOLUME_MASK:
        vols, tfs = vt.scene(variant, n=n)
        return vols, tfs[1:]
    vols, _ = vt.scene(variant, n=n)
    return vols, []


def load(ctx, vols, tf0, other):
    for i, v in enumerate(vols):
        ctx.volume_upload(i, v)
    for i, t in enumerate([tf0] + list(other)):
        ctx.tf_upload(i, t[0], t[1])


def cameras(W, H, n):
    step, count = hr.stepping_params(n, n, n)
    return [hr.make_uniforms(W, H, steps_count=count, step_size=step, distance=0.9 + 0.1 * k, yaw=0.4 * k, pitch=0.3 - 0.2 * k)
            for k in range(4)]


T0 = prefix_tf(64, 9)
EDITS = {"prefix_up": prefix_tf(64, 20), "prefix_down": prefix_tf(64, 3), "colour_only": recolour(T0),
         "resolution": prefix_tf(128, 30)}


@pytest.mark.parametrize("variant", [capi.LIGHT, capi.BASIC, capi.VOLUME_MASK])
def test_edits_are_ordered_across_streams(variant):
    """Two frames, an edit, three frames on other streams, no waits in between: every frame equals the cold render of the table
    it was enqueued under; the last launch's counters equal the cold ones (flavour 17 in both)."""
    n, W, H = 24, 160, 96
    vols, other = setup(variant, n)
    us = cameras(W, H, n)
    cold = Cold(variant, vols, other, W, H, 17)
    outs = [capi.Context(W, H, 0) for _ in range(5)]
    try:
        with capi.Context(W, H, 0) as ctx:
            ctx.set_kernel_flavour(17)
            load(ctx, vols, T0, other)
            st = [ctx.stream(k) for k in range(4)]
            cases = [(name, tf, 0) for name, tf in EDITS.items()] + [("own_stream", EDITS["prefix_up"], st[1])]
            for name, tf, edit_stream in cases:
                ctx.tf_upload(0, T0[0], T0[1])  # (synchronous: the field of T0 exists)
                ctx.set_uniforms(vt.to_capi_uniforms(us[0]))
                ctx.render(variant)
                plan = [(us[0], st[0], T0), (us[1], st[1], T0), None, (us[2], st[2], tf), (us[3], st[3], tf), (us[0], st[0], tf)]
                k = 0
                for step in plan:
                    if step is None:
                        o = tf[0].copy()
                        c = tf[1].copy()
                        ctx.tf_upload_async(0, opacity=o, color=c, stream=edit_stream)
                        o[:] = 1.0  # (copied on call: the caller's arrays may change at once)
                        c[:] = 1.0
                        continue
                    ctx.set_uniforms(vt.to_capi_uniforms(step[0]))
                    ctx.render_async(variant, outs[k].frame_device_ptr(), step[1])
                    k += 1
                got_counters = ctx.counters()
                ctx.resize(W, H)  # (drains the device)
                k = 0
                for step in plan:
                    if step is None:
                        continue
                    ref = cold(step[2], step[0])
                    got, _, _ = outs[k].download()
                    assert np.array_equal(vt.bits(got), vt.bits(ref[0])), (name, k)
                    k += 1
                assert got_counters == cold(tf, us[0])[1], name
    finally:
        for o in outs:
            o.close()
        cold.close()


@pytest.mark.parametrize("flavour", [0, 1, 6, 7, 8, 10, 11, 12, 13, 15, 16, 17, 18])
def test_every_kernel_form_after_an_edit(flavour):
    n, W, H = 24, 160, 96
    vols, other = setup(capi.LIGHT, n)
    u = cameras(W, H, n)[1]
    tf = prefix_tf(64, 17)
    cold = Cold(capi.LIGHT, vols, other, W, H, flavour)
    out = capi.Context(W, H, 0)
    try:
        with capi.Context(W, H, 0) as ctx:
            ctx.set_kernel_flavour(flavour)
            load(ctx, vols, T0, other)
            ctx.set_uniforms(vt.to_capi_uniforms(u))
            ctx.render(capi.LIGHT)
            ctx.tf_upload_async(0, opacity=tf[0], color=tf[1], stream=ctx.stream(0))
            ctx.render_async(capi.LIGHT, out.frame_device_ptr(), ctx.stream(1))
            ctx.resize(W, H)
            ref = cold(tf, u)
            got, _, _ = out.download()
            assert np.array_equal(vt.bits(got), vt.bits(ref[0]))
            assert ctx.last_kernel_flavour() == ref[2]
    finally:
        out.close()
        cold.close()


def test_a_drag_of_64_edits():
    """The reference's drag (OpacityTF::UpdateYAxis): the first non-zero texel moves by one per frame; 64 edits, each followed at
    once by a frame on stream k & 3, no host wait -- more than the tables' and the field's generations hold."""
    n, W, H = 24, 128, 80
    vols, other = setup(capi.LIGHT, n)
    us = cameras(W, H, n)
    cold = Cold(capi.LIGHT, vols, other, W, H, 17)
    big = capi.Context(W, H * 64, 0)  # (64 output frames, one after the other)
    try:
        with capi.Context(W, H, 0) as ctx:
            ctx.set_kernel_flavour(17)
            load(ctx, vols, T0, other)
            ctx.set_uniforms(vt.to_capi_uniforms(us[0]))
            ctx.render(capi.LIGHT)
            st = [ctx.stream(k) for k in range(4)]
            base = big.frame_device_ptr()
            tfs = [prefix_tf(128, 4 + k) for k in range(64)]
            miss0 = ctx.unbounded_box_launches()
            for k in range(64):
                ctx.tf_upload_async(0, opacity=tfs[k][0], color=tfs[k][1], stream=st[k & 3] if k % 2 else 0)
                ctx.set_uniforms(vt.to_capi_uniforms(us[k & 3]))
                ctx.render_async(capi.LIGHT, base + k * W * H * 16, st[k & 3])
            got_counters = ctx.counters()
            # (frames enqueued right behind an edit run before its field's box has reached the host: the unbounded box was used)
            assert ctx.unbounded_box_launches() > miss0
            ctx.resize(W, H)
            frames, _, _ = big.download()
            for k in range(64):
                ref = cold(tfs[k], us[k & 3])
                assert np.array_equal(vt.bits(frames[k * H:(k + 1) * H]), vt.bits(ref[0])), k
            assert got_counters == cold(tfs[63], us[3])[1]
    finally:
        big.close()
        cold.close()


def _hip():
    capi.load()
    return C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))


def test_an_edit_does_not_drain_the_device():
    """Work on all four streams, then an edit that moves the zero prefix and changes the resolution, then a frame: at least one of
    the four streams must still be busy (hipStreamQuery), which a draining edit cannot leave behind."""
    hip = _hip()
    hip.hipStreamQuery.argtypes = [C.c_void_p]
    n, W, H = 64, 1920, 1080
    vols, other = setup(capi.LIGHT, n)
    thin = prefix_tf(256, 8, top=0.002)
    step, count = hr.stepping_params(n, n, n)
    outs = [capi.Context(W, H, 0) for _ in range(4)]
    try:
        with capi.Context(W, H, 0) as ctx:
            ctx.set_kernel_flavour(17)
            load(ctx, vols, thin, other)
            st = [ctx.stream(k) for k in range(4)]
            ctx.tf_upload_async(0, opacity=thin[0], color=thin[1])  # (warm: the staging exists)

            def batch(scale):
                return [vt.to_capi_uniforms(hr.make_uniforms(W, H, steps_count=count * scale, step_size=step / scale, yaw=0.3 * f))
                        for f in range(4)]
            bufs = [o.frame_device_ptr() for o in outs]
            t0 = time.perf_counter()
            ctx.render_batch_async(capi.LIGHT, batch(1), bufs, st[0])
            ctx.counters()
            ms1 = (time.perf_counter() - t0) * 1e3
            scale = int(min(64, max(1, np.ceil(8.0 / max(ms1, 1e-3)))))
            ctx.render_batch_async(capi.LIGHT, batch(scale), bufs, st[0])
            t0 = time.perf_counter()
            ctx.render_batch_async(capi.LIGHT, batch(scale), bufs, st[0])
            ctx.counters()
            ms = (time.perf_counter() - t0) * 1e3
            print(f"one batched launch: {ms:.1f} ms ({scale}x steps); 7 enqueued: about {7 * ms:.0f} ms of device work")
            assert 7 * ms > 10.0
            for k in range(7):
                ctx.render_batch_async(capi.LIGHT, batch(scale), bufs, st[k & 3])
            edit = prefix_tf(512, 40, top=0.002)
            ctx.tf_upload_async(0, opacity=edit[0], color=edit[1])
            ctx.set_uniforms(vt.to_capi_uniforms(hr.make_uniforms(W, H, steps_count=count, step_size=step)))
            ctx.render_async(capi.LIGHT, 0, 0)
            busy = [hip.hipStreamQuery(C.c_void_p(s)) for s in st]
            assert any(b != 0 for b in busy), busy
            ctx.resize(W, H)
    finally:
        for o in outs:
            o.close()


def test_a_generation_outlives_readers_on_other_streams():
    """A long batched frame on stream 0 and a short frame on stream 1, both under T0; then four asynchronous edits on stream 1 that
    move the zero prefix -- the fourth rewrites T0's table generation and the field generation both frames read.  It must wait for
    the long frame as well, not only for the newest reader: every frame of the long launch equals its cold T0 render."""
    n, W, H = 64, 960, 540
    vols, other = setup(capi.LIGHT, n)
    t0 = prefix_tf(256, 8, top=0.002)
    step, count = hr.stepping_params(n, n, n)
    cold = Cold(capi.LIGHT, vols, other, W, H, 17)
    outs = [capi.Context(W, H, 0) for _ in range(5)]
    try:
        with capi.Context(W, H, 0) as ctx:
            ctx.set_kernel_flavour(17)
            load(ctx, vols, t0, other)
            st = [ctx.stream(k) for k in range(4)]
            bufs = [o.frame_device_ptr() for o in outs[:4]]

            def batch(scale):
                return [hr.make_uniforms(W, H, steps_count=count * scale, step_size=step / scale, yaw=0.3 * f) for f in range(4)]
            tm = time.perf_counter()
            ctx.render_batch_async(capi.LIGHT, [vt.to_capi_uniforms(u) for u in batch(1)], bufs, st[0])
            ctx.counters()
            ms1 = (time.perf_counter() - tm) * 1e3
            scale = int(min(64, max(1, np.ceil(10.0 / max(ms1, 1e-3)))))
            us = batch(scale)
            ctx.render_batch_async(capi.LIGHT, [vt.to_capi_uniforms(u) for u in us], bufs, st[0])  # the long reader
            small = hr.make_uniforms(W, H, steps_count=4, step_size=step)
            ctx.set_uniforms(vt.to_capi_uniforms(small))
            ctx.render_async(capi.LIGHT, outs[4].frame_device_ptr(), st[1])  # the newest reader, soon done
            for k in range(4):
                t = prefix_tf(256, 20 + 10 * k, top=0.5)
                ctx.tf_upload_async(0, opacity=t[0], color=t[1], stream=st[1])
            ctx.resize(W, H)
            for f in range(4):
                got, _, _ = outs[f].download()
                assert np.array_equal(vt.bits(got), vt.bits(cold(t0, us[f])[0])), f
            got, _, _ = outs[4].download()
            assert np.array_equal(vt.bits(got), vt.bits(cold(t0, small)[0]))
    finally:
        for o in outs:
            o.close()
        cold.close()


def spot_volume(shape, spots):
    nz, ny, nx = shape
    v = np.zeros((nz, ny, nx, 4), dtype=f32)
    for (z, y, x) in spots:
        v[z:z + 4, y:y + 4, x:x + 4, 3] = 1.0
    return v


@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("length", [4, 148, 1100])
@pytest.mark.parametrize("case", ["none", "all", "spots"])
def test_field_matches_numpy(axis, length, case):
    """Brick grids of 1, 37 and 275 bricks along one axis: no active brick, all bricks active, and hand-placed dense bricks whose
    distances reach the cap.  The field, box and count equal numpy's, after a synchronous upload and after an asynchronous edit
    back to the same table."""
    shape = [8, 8, 8]
    shape[2 - axis] = length
    shape = tuple(shape)
    if case == "all":
        vol = np.full(shape + (4,), 1.0, dtype=f32)
    elif case == "none":
        vol = np.zeros(shape + (4,), dtype=f32)
    else:
        far = [0, 0, 0]
        far[2 - axis] = length - 4
        vol = spot_volume(shape, [(0, 0, 0), tuple(far)] if length > 600 else [(0, 0, 0)])
    tf, tf2 = prefix_tf(64, 9), prefix_tf(64, 30)
    with capi.Context(64, 64, 0) as ctx:
        ctx.volume_upload(0, vol)
        ctx.tf_upload(0, *tf)
        f1 = check_field(ctx, capi.BASIC, numpy_active(vol, tf[0]))
        if case == "none":
            assert f1[2] == 0 and (f1[0] == CAP).all()
        if case == "all":
            assert (f1[0] == 0).all()
        if case == "spots":
            assert f1[0][0, 0, 0] == 0 and (length < 600 or f1[0].max() == CAP)
        ctx.tf_upload(0, *tf2)
        check_field(ctx, capi.BASIC, numpy_active(vol, tf2[0]))
        ctx.tf_upload_async(0, opacity=tf[0], color=tf[1], stream=ctx.stream(1))
        f2 = check_field(ctx, capi.BASIC, numpy_active(vol, tf[0]))
        assert np.array_equal(f1[0], f2[0]) and f1[1:] == f2[1:]


def test_field_of_the_merged_records():
    """VOLUME_MASK (C4's shape, small): the field over the merged mask / CT records."""
    vols, tfs = vt.scene(capi.VOLUME_MASK, n=48)
    with capi.Context(64, 64, 0) as ctx:
        for i, v in enumerate(vols):
            ctx.volume_upload(i, v)
        ctx.tf_upload(0, *prefix_tf(64, 9))
        ctx.tf_upload(1, *tfs[1])
        f1 = check_field(ctx, capi.VOLUME_MASK, numpy_active(vols[2], prefix_tf(64, 9)[0], vols[0]))
        assert 0 < f1[2] < f1[0].size
        ctx.tf_upload(0, *prefix_tf(64, 40))
        check_field(ctx, capi.VOLUME_MASK, numpy_active(vols[2], prefix_tf(64, 40)[0], vols[0]))
        t = prefix_tf(64, 9)
        ctx.tf_upload_async(0, opacity=t[0], color=t[1])
        f2 = check_field(ctx, capi.VOLUME_MASK, numpy_active(vols[2], t[0], vols[0]))
        assert np.array_equal(f1[0], f2[0]) and f1[1:] == f2[1:]


def test_bad_edits_are_rejected():
    n, W, H = 24, 96, 64
    vols, other = setup(capi.LIGHT, n)
    u = cameras(W, H, n)[0]
    cold = Cold(capi.LIGHT, vols, other, W, H, 0)
    try:
        with capi.Context(W, H, 0) as ctx:
            load(ctx, vols, T0, other)
            lib, o = ctx.lib, T0[0]
            for fn, per in ((lib.vr_tf_upload_opacity_async, 1), (lib.vr_tf_upload_color_async, 4)):
                t = np.ones(64 * per, dtype=f32)
                assert fn(ctx.h, -1, t.ctypes.data, 64, None) == capi.VR_ERR_INVALID_ARG
                assert fn(ctx.h, 2, t.ctypes.data, 64, None) == capi.VR_ERR_INVALID_ARG
                assert fn(ctx.h, 0, None, 64, None) == capi.VR_ERR_INVALID_ARG
                assert fn(ctx.h, 0, t.ctypes.data, 0, None) == capi.VR_ERR_INVALID_ARG
                assert fn(ctx.h, 0, t.ctypes.data, (1 << 24) + 1, None) == capi.VR_ERR_INVALID_ARG
            assert o is T0[0]
            ctx.set_uniforms(vt.to_capi_uniforms(u))
            ctx.render(capi.LIGHT)
            got, _, _ = ctx.download()
            assert np.array_equal(vt.bits(got), vt.bits(cold(T0, u)[0]))
    finally:
        cold.close()
