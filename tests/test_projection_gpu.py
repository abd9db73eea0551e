"""GPU side of the intensity projections (VR_VARIANT_MIP / MINIP / AVERAGE, csrc/vr_proj.h): frames and counters bit-exact against
the float32 restatement (proj_ref.py, itself pinned to the oracle's BASIC march by tests/test_projection.py), the same bits from
every kernel form, layout, launch shape and arithmetic check, hostile volumes, volume edits, and no interference with the
compositing shaders."""
import numpy as np
import pytest

import host_ref as hr
import oracle_binding as ob
import proj_ref as pr
import vrtest as vt
from volumerendering_amd import capi

pytestmark = pytest.mark.gpu
f32 = np.float32
MODES = [capi.MIP, capi.MINIP, capi.AVERAGE]
W, H = 72, 56


def phantom(n=16):
    return vt.make_volume("phantom", n)


def tf_pair(res=64):
    return hr.default_opacity_tf(res), hr.default_color_tf(res)


def uniforms(shape, **over):
    step, count = hr.stepping_params(*shape)
    kw = dict(steps_count=count, step_size=step)
    kw.update(over)
    return hr.make_uniforms(W, H, **kw)


def render(ctx, variant, u, v, tf):
    frag, _, _ = vt.gpu_render(ctx, variant, u, [v], [tf])
    return frag, ctx.counters()


def air_and_core(n=24):
    """Exact-zero air around a bright core: most bricks are inert for every mode."""
    v = np.zeros((n, n, n, 4), f32)
    c = n // 2
    v[c - 3:c + 3, c - 3:c + 3, c - 3:c + 3, 3] = f32(0.9)
    v[c - 1:c + 1, c - 1:c + 1, c - 1:c + 1, 3] = f32(1.0)
    return v


CASES = [
    ("sphere", lambda: vt.make_volume("sphere", 16), 64, {}),
    ("phantom", phantom, 16, {}),
    ("aniso", lambda: ob.normalize_data(hr.raw_to_vec4(np.random.default_rng(7).integers(0, 4096, size=(7, 20, 13)).astype(np.uint16))),
     257, {}),
    ("clip", phantom, 64, dict(clip_x=(0.1, 0.2), clip_y=(0.05, 0.0), clip_z=(0.0, 0.3))),
    ("varstep", phantom, 64, dict(toggles=(1, 0, 0, 0))),
    ("jitter", lambda: vt.make_volume("sphere", 16), 64, dict(toggles=(0, 1, 0, 0))),
    ("steps0", phantom, 64, dict(steps_count=0)),
    ("steps1", phantom, 64, dict(steps_count=1)),
    ("steps7", phantom, 64, dict(steps_count=7, step_size=0.05)),
    ("core", air_and_core, 64, {}),
]


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(W, H, 0)
    yield c
    c.close()


@pytest.mark.parametrize("variant", MODES)
@pytest.mark.parametrize("cid,make,res,over", CASES, ids=[c[0] for c in CASES])
def test_matches_restatement(ctx, variant, cid, make, res, over):
    v, tf = make(), tf_pair(res)
    u = uniforms((v.shape[2], v.shape[1], v.shape[0]), **over)
    ref, n_ref, cov_ref = pr.frame(variant, u, W, H, v, tf)
    for fl in (0, 1):
        ctx.set_kernel_flavour(fl)
        frag, (n, cov, fetched) = render(ctx, variant, u, v, tf)
        assert ctx.last_kernel_flavour() == (19 if fl == 0 else 20)
        assert np.array_equal(vt.bits(frag), vt.bits(ref)), (fl, float(np.nanmax(np.abs(frag - ref))))
        assert (n, cov) == (n_ref, cov_ref)
        assert fetched <= n and (fl == 0 or fetched == n)
    ctx.set_kernel_flavour(0)


@pytest.mark.parametrize("variant", MODES)
def test_forms_layouts_and_skipping(ctx, variant):
    """Flavours 0 / 1 x layouts 0 / 1 / 3 give the same bits; on exact-zero air around a bright core the skipping form fetches
    fewer samples than it counts; the MIP of that core reaches the volume's maximum and exits early, still exact."""
    v, tf = air_and_core(), tf_pair()
    u = uniforms((24, 24, 24))
    ref, n_ref, cov_ref = pr.frame(variant, u, W, H, v, tf)
    fetched = {}
    for layout in (0, 1, 3):
        ctx.set_volume_layout(layout)
        for fl in (0, 1):
            ctx.set_kernel_flavour(fl)
            frag, (n, cov, f) = render(ctx, variant, u, v, tf)
            assert np.array_equal(vt.bits(frag), vt.bits(ref)), (layout, fl)
            assert (n, cov) == (n_ref, cov_ref)
            fetched[layout, fl] = f
    ctx.set_volume_layout(0)
    ctx.set_kernel_flavour(0)
    assert fetched[0, 0] < n_ref and fetched[0, 1] == n_ref
    if variant == capi.MIP:
        # early exit: the rays through the core stop loading at its maximum (1.0) -- fewer loads than skipping by bricks alone
        # would leave, as the core's own bricks are never inert
        assert fetched[0, 0] < fetched[0, 1] // 4


@pytest.mark.parametrize("variant", MODES)
def test_fused_arithmetic(ctx, variant):
    """VR_ARITH_FUSED: every form and layout gives the same bits, within the float64 tolerance of the separate frame -- and they are
    the bits of the fused restatement (proj_ref.frame(fused=True): the sampler's and look-up's coordinates and lerps and the blend
    fused, positions and AVERAGE's sum and mean not), with its counters."""
    v, tf = phantom(), tf_pair()
    u = uniforms((16, 16, 16))
    ref, n_ref, _ = pr.frame(variant, u, W, H, v, tf)
    fref, n_fref, cov_fref = pr.frame(variant, u, W, H, v, tf, fused=True)
    # (the two modes part company on this frame; MINIP's minimum is the air's exact 0 in both)
    assert variant == capi.MINIP or not np.array_equal(vt.bits(fref), vt.bits(ref))
    ctx.set_arithmetic(capi.ARITH_FUSED)
    try:
        frames = []
        for layout in (0, 1, 3):
            ctx.set_volume_layout(layout)
            for fl in (0, 1):
                ctx.set_kernel_flavour(fl)
                frag, (n, _, _) = render(ctx, variant, u, v, tf)
                assert n == n_ref
                frames.append(frag)
        for f in frames[1:]:
            assert np.array_equal(vt.bits(f), vt.bits(frames[0]))
        assert float(np.max(np.abs(frames[0] - ref))) <= 1e-3
        assert np.array_equal(vt.bits(frames[0]), vt.bits(fref)), float(np.nanmax(np.abs(frames[0] - fref)))
        assert ctx.counters()[:2] == (n_fref, cov_fref)
    finally:
        ctx.set_arithmetic(capi.ARITH_SEPARATE)
        ctx.set_volume_layout(0)
        ctx.set_kernel_flavour(0)


def hostile_volumes():
    v = phantom()
    nan = v.copy()
    nan[5, 7, 8, 3] = np.nan
    inf = v.copy()
    inf[8, 8, 8, 3] = np.inf
    inf[3, 9, 4, 3] = -np.inf
    return [("nan", nan), ("inf", inf), ("zero", np.zeros_like(v))]


@pytest.mark.parametrize("variant", MODES)
def test_hostile_inputs(ctx, variant):
    """NaN and +-inf voxels, an all-zero volume, zero steps, rays that miss the box and a clip that empties it: flavours 0 and 1
    agree with the restatement bit for bit (NaN where it is NaN)."""
    tf = tf_pair()
    cases = [(name, v, {}) for name, v in hostile_volumes()]
    cases += [("steps0", phantom(), dict(steps_count=0)), ("miss", phantom(), dict(distance=6.0, yaw=2.2, pitch=1.4, fov_deg=3.0)),
              ("clip_all", phantom(), dict(clip_x=(0.6, 0.6)))]
    for name, v, over in cases:
        u = uniforms((16, 16, 16), **over)
        ref, n_ref, cov_ref = pr.frame(variant, u, W, H, v, tf)
        for fl in (0, 1):
            ctx.set_kernel_flavour(fl)
            frag, (n, cov, _) = render(ctx, variant, u, v, tf)
            assert np.array_equal(np.isnan(frag), np.isnan(ref)), (name, fl)
            fin = ~np.isnan(ref)
            assert np.array_equal(vt.bits(frag)[fin], vt.bits(ref)[fin]), (name, fl)
            assert (n, cov) == (n_ref, cov_ref), (name, fl)
        if name == "clip_all":
            assert n_ref == 0 and not np.any(ref)
    ctx.set_kernel_flavour(0)


def test_tiles_and_batches(ctx):
    """Tiles of world 2 / 3 / 8, unpacked, equal the frame; a batch of frames equals the single renders."""
    v, tf = phantom(), tf_pair()
    us = [uniforms((16, 16, 16), yaw=0.6 + 0.4 * k, clip_z=(0.0, 0.1 * k)) for k in range(4)]
    for variant in MODES:
        refs = [vt.gpu_render(ctx, variant, u, [v], [tf])[0] for u in us]
        ctx.set_uniforms(vt.to_capi_uniforms(us[0]))
        for world in (2, 3, 8):
            full = np.zeros((H, W, 4), f32)
            for rank in range(world):
                cnt = ctx.tile_count(rank, world)
                ctx.render_tiles(variant, rank, world)
                if cnt == 0:
                    continue
                tl, _ = ctx.download_tiles(cnt)
                tl = tl.reshape(cnt, capi.TILE, capi.TILE, 4)
                tiles_x = (W + capi.TILE - 1) // capi.TILE
                for n in range(cnt):
                    t = rank + n * world
                    ty, tx = divmod(t, tiles_x)
                    y0, x0 = ty * capi.TILE, tx * capi.TILE
                    h, w = min(capi.TILE, H - y0), min(capi.TILE, W - x0)
                    full[y0:y0 + h, x0:x0 + w] = tl[n, :h, :w]
            assert np.array_equal(vt.bits(full), vt.bits(refs[0])), (variant, world)
        others = [capi.Context(W, H, 0) for _ in range(4)]
        try:
            ctx.render_batch_async(variant, [vt.to_capi_uniforms(u) for u in us], [o.frame_device_ptr() for o in others], ctx.stream(0))
            ctx.counters()
            for o, r in zip(others, refs):
                got, _, _ = o.download()
                assert np.array_equal(vt.bits(got), vt.bits(r)), variant
        finally:
            for o in others:
                o.close()


def test_streams_and_async_opacity_edit():
    """Two streams in flight give the single renders; an asynchronous opacity edit followed by a projection equals a cold render
    with the edited table."""
    v, tf = phantom(), tf_pair()
    u = uniforms((16, 16, 16))
    with capi.Context(W, H, 0) as ctx, capi.Context(W, H, 0) as o0, capi.Context(W, H, 0) as o1:
        ref = vt.gpu_render(ctx, capi.MIP, u, [v], [tf])[0]
        ref_avg = vt.gpu_render(ctx, capi.AVERAGE, u, [v], [tf])[0]
        for _ in range(3):
            ctx.render_async(capi.MIP, o0.frame_device_ptr(), ctx.stream(0))
            ctx.render_async(capi.AVERAGE, o1.frame_device_ptr(), ctx.stream(1))
        ctx.counters()  # (waits for the last launch; the first stream's are older and done by the end of the copy below)
        assert np.array_equal(vt.bits(o0.download()[0]), vt.bits(ref))
        assert np.array_equal(vt.bits(o1.download()[0]), vt.bits(ref_avg))
        edited = (hr.thin_opacity_tf(64, 0.5), tf[1])
        ctx.tf_upload_async(0, opacity=edited[0], stream=ctx.stream(1))
        ctx.render_async(capi.MIP, o0.frame_device_ptr(), ctx.stream(1))
        ctx.counters()
        with capi.Context(W, H, 0) as cold:
            want = vt.gpu_render(cold, capi.MIP, u, [v], [edited])[0]
        assert np.array_equal(vt.bits(o0.download()[0]), vt.bits(want))


def test_volume_edit_rebuilds_ranges(ctx):
    """After vr_volume_upload of a volume whose maximum moved, the brick ranges are rebuilt and the MIP still matches."""
    tf = tf_pair()
    u = uniforms((24, 24, 24))
    a = air_and_core()
    b = air_and_core()
    b[..., 3] *= f32(0.5)
    b[2:5, 3:6, 18:21, 3] = f32(1.0)
    for v in (a, b, a):
        ctx.set_kernel_flavour(0)
        frag, (n, cov, _) = render(ctx, capi.MIP, u, v, tf)
        ref, n_ref, cov_ref = pr.frame(capi.MIP, u, W, H, v, tf)
        assert np.array_equal(vt.bits(frag), vt.bits(ref))
        assert (n, cov) == (n_ref, cov_ref)


def test_no_interference_and_choice():
    """LIGHT frames and vr_skip_field are bit-identical before and after projection launches; a projection has no measured
    choice and no distance field."""
    vl, tfl = vt.scene(capi.LIGHT, n=16)
    u = uniforms((16, 16, 16))
    with capi.Context(W, H, 0) as ctx:
        before = vt.gpu_render(ctx, capi.LIGHT, u, vl, tfl)
        field0 = ctx.skip_field(capi.LIGHT)
        for variant in MODES:
            ctx.render(variant)
            assert ctx.kernel_choice()[0] == [] and ctx.last_kernel_flavour() == 19
            with pytest.raises(capi.VrError) as e:
                ctx.skip_field(variant)
            assert e.value.code == capi.VR_ERR_NOT_READY
        after = vt.gpu_render(ctx, capi.LIGHT, u, vl, tfl)
        field1 = ctx.skip_field(capi.LIGHT)
        assert np.array_equal(vt.bits(before[0]), vt.bits(after[0])) and before[2] == after[2]
        assert all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(field0, field1))


@pytest.mark.parametrize("variant", [capi.MIP, capi.AVERAGE])
def test_c3_seeded_pixels(variant):
    """Full size, through the host surface: C3's 512^3 phantom at 1920 x 1080 started as a ProjectionApp
    (host.Application.OnStart(MIP / AVERAGE, ...)), 2 048 seeded pixels of the frame exact against the restatement."""
    from volumerendering_amd import host, synth, workloads as wl
    n, W3, H3, _ = wl.WORKLOADS["C3"]
    with host.Application(W3, H3, 0) as app:
        vol = host.VolumeFile.from_raw(synth.ct_phantom_raw_fast(n))
        app.OnStart(variant, [vol])
        app.camera().SetOrbit(*wl.CAMERA)
        app.OnUpdate()
        app.OnRender()
        frag, _, samples = app.ReadFrame()
        ub, volumes, tfs = wl.oracle_inputs(app, [vol])
        assert app.context().last_kernel_flavour() == 19
    u = hr.Uniforms.from_buffer_copy(ub)
    rng = np.random.default_rng(2048)
    pix = np.stack([rng.integers(0, W3, 2048), rng.integers(0, H3, 2048)], 1)
    ref, comp, cov, _ = pr.march(variant, u, W3, H3, volumes[0], tfs[0], pix)
    got = frag[pix[:, 1], pix[:, 0]]
    assert cov.sum() > 500 and samples > 0
    assert np.array_equal(vt.bits(got), vt.bits(ref)), float(np.nanmax(np.abs(got - ref)))
