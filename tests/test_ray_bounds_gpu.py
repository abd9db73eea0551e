"""GPU side of the per-pixel ray bounds (vr_set_ray_bounds, csrc/vr_bound.h): frames and counters bit-exact against the float32
restatement (bound_ref.py, itself pinned to the oracle by tests/test_ray_bounds.py) for BASIC and LIGHT, flavours 27 and 28, with a
near bound, a far bound, both, the round-trip depth of a surface frame and hostile values; the fused mode against the oracle's fused
frames through the trivial-bound and steps_count = m pins; the same bits from every layout and launch shape; the feature's reason (a
LIGHT frame cut by the ISO surface's own depth, computed on the device); and no interference with anything else."""
import ctypes as C
import os

import numpy as np
import pytest

import bound_ref as br
import feature_cases as fc
import host_ref as hr
import iso_ref as ir
import oracle_binding as ob
import surf_ref as sr
import vrtest as vt
from volumerendering_amd import capi

pytestmark = pytest.mark.gpu
f32 = np.float32
W, H = 72, 56


def _hip():
    try:
        return C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
    except OSError:
        return C.CDLL("libamdhip64.so")  # the runtime libvr_hip.so itself is linked against


class DevBuf:
    """W*H floats of device memory, written and read with synchronous copies (ordered before every later launch)."""

    def __init__(self, hip, values=None):
        self.hip, self.p = hip, C.c_void_p()
        assert hip.hipMalloc(C.byref(self.p), C.c_size_t(W * H * 4)) == 0
        if values is not None:
            self.write(values)

    @property
    def ptr(self):
        return int(self.p.value)

    def write(self, values):
        a = np.ascontiguousarray(values, dtype=f32).reshape(H, W)
        assert self.hip.hipMemcpy(self.p, a.ctypes.data_as(C.c_void_p), C.c_size_t(a.nbytes), 1) == 0  # hipMemcpyHostToDevice
        return self

    def read(self):
        a = np.empty((H, W), f32)
        assert self.hip.hipMemcpy(a.ctypes.data_as(C.c_void_p), self.p, C.c_size_t(a.nbytes), 2) == 0  # hipMemcpyDeviceToHost
        return a

    def free(self):
        if self.p:
            self.hip.hipFree(self.p)
            self.p = C.c_void_p()


@pytest.fixture(scope="module")
def hip():
    return _hip()


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(W, H, 0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def bufs(hip, ctx):  # (after the context: the device is the one it opened)
    b = [DevBuf(hip), DevBuf(hip)]
    yield b
    for x in b:
        x.free()


def phantom(n=16):
    return vt.make_volume("phantom", n, gradient=True)


def steep_tf(res=64, gain=4.0):
    """Opacity min(1, gain * ramp), exactly 0 at density 0 (tests/test_surface.py checks on the CPU that rays reach the cut-offs)."""
    return np.minimum(hr.default_opacity_tf(res) * f32(gain), f32(1.0)).astype(f32), hr.default_color_tf(res)


def air_and_core(n=24):
    """Exact-zero air around a bright core (gradient in .rgb): most bricks are inert under any table with opacity[0] == 0."""
    v = np.zeros((n, n, n, 4), f32)
    c = n // 2
    v[c - 3:c + 3, c - 3:c + 3, c - 3:c + 3, 3] = f32(0.9)
    v[c - 1:c + 1, c - 1:c + 1, c - 1:c + 1, 3] = f32(1.0)
    return ob.precompute_gradient(v)


def uniforms(shape, **over):
    step, count = hr.stepping_params(*shape)
    kw = dict(steps_count=count, step_size=step)
    kw.update(over)
    return hr.make_uniforms(W, H, **kw)


def shape_of(v):
    return v.shape[2], v.shape[1], v.shape[0]


def plane(value):
    return np.full((H, W), value, f32)


def seeded_depth(u, seed):
    lo, hi = br.box_corner_depths(u)
    return (lo + (hi - lo) * np.random.default_rng(seed).random((H, W), dtype=np.float32)).astype(f32)


def hostile(u, seed):
    """A buffer that cycles through NaN, +-inf, -1, 2 and two ordinary depths, shuffled per seed."""
    lo, hi = br.box_corner_depths(u)
    vals = np.array([np.nan, np.inf, -np.inf, -1.0, 2.0, lo + (hi - lo) * 0.4, lo + (hi - lo) * 0.6], f32)
    return vals[np.random.default_rng(seed).integers(0, len(vals), size=(H, W))]


def bind(ctx, bufs, near, far):
    """Writes the two depth buffers (None = no bound on that side) and binds them."""
    ctx.set_ray_bounds(bufs[0].write(near).ptr if near is not None else None, bufs[1].write(far).ptr if far is not None else None)


def bounded(ctx, bufs, variant, u, v, tf, near, far, flavour=0):
    """A bounded frame and its counters; bounds and flavour are put back."""
    bind(ctx, bufs, near, far)
    ctx.set_kernel_flavour(flavour)
    try:
        frag, _, _ = vt.gpu_render(ctx, variant, u, [v], [tf])
        return frag, ctx.counters(), ctx.last_kernel_flavour(), ctx.kernel_choice()[0]
    finally:
        ctx.set_kernel_flavour(0)
        ctx.set_ray_bounds(None, None)


def bound_sets(u, v, tf):
    """(name, near, far): near only, far only, both (some pixels with near > far), the round-trip depth, the hostile set."""
    s = sr.march(u, W, H, v, tf[0], 0.5)
    centre = plane(br.depth_of_world(u, (0.0, 0.0, 0.0)))
    return [("near", seeded_depth(u, 1), None), ("far", None, seeded_depth(u, 2)), ("both", seeded_depth(u, 3), centre),
            ("round trip", None, sr.depth(s["frag"], u, 0.5).reshape(H, W)), ("hostile near", hostile(u, 4), None),
            ("hostile far", None, hostile(u, 5)), ("hostile both", hostile(u, 6), hostile(u, 7))]


CASES = [
    ("phantom", phantom, 64, {}),
    ("sphere", lambda: vt.make_volume("sphere", 16, gradient=True), 16, {}),
    ("clip", phantom, 64, dict(clip_x=(0.1, 0.2), clip_y=(0.05, 0.0), clip_z=(0.0, 0.3))),
    ("varstep", phantom, 64, dict(toggles=(1, 0, 0, 0))),
    ("jitter", lambda: vt.make_volume("sphere", 16, gradient=True), 64, dict(toggles=(0, 1, 0, 0))),
    ("steps1", phantom, 64, dict(steps_count=1)),
    ("steps7", phantom, 64, dict(steps_count=7, step_size=0.05)),
    ("core", air_and_core, 64, {}),
]


@pytest.mark.parametrize("cid,make,res,over", CASES, ids=[c[0] for c in CASES])
def test_matches_restatement(ctx, bufs, cid, make, res, over):
    """Frames and counters of flavours 27 and 28, BASIC and LIGHT, against the restatement for every bound set."""
    v, tf = make(), steep_tf(res)
    u = uniforms(shape_of(v), **over)
    for name, near, far in bound_sets(u, v, tf):
        for variant in (capi.BASIC, capi.LIGHT):
            ref, n_ref, cov_ref = br.frame(variant, u, W, H, v, tf, near, far)
            for fl in (0, 1):
                frag, (n, cov, f), ran, cand = bounded(ctx, bufs, variant, u, v, tf, near, far, fl)
                print(cid, name, variant, fl, "composited", n, "ref", n_ref, "fetched", f)
                assert ran == (28 if fl == 1 else 27) and cand == []
                assert np.array_equal(vt.bits(frag), vt.bits(ref)), (name, variant, fl, float(np.nanmax(np.abs(frag - ref))))
                assert (n, cov) == (n_ref, cov_ref), (name, variant, fl)
                assert f <= n and (fl == 0 or f == n)
    if cid == "phantom":
        free = br.frame(capi.LIGHT, u, W, H, v, tf)
        assert br.frame(capi.LIGHT, u, W, H, v, tf, None, seeded_depth(u, 2))[1] < free[1]  # (the far set does cut)


@pytest.mark.parametrize("mode", [capi.ARITH_SEPARATE, capi.ARITH_FUSED], ids=["separate", "fused"])
@pytest.mark.parametrize("variant", [capi.BASIC, capi.LIGHT], ids=["basic", "light"])
def test_pins_to_the_oracle_in_both_arithmetic_modes(ctx, bufs, mode, variant):
    """near = 0, far = 1 is the oracle's frame; a far bound that leaves the steps 0 .. m-1 is the pixel of the oracle's frame with
    steps_count = m (m from the restatement: ray placement, the same in both modes).  And the restatement of the mode
    (bound_ref.frame(fused=...)): the far-bounded frame and one between a near and a far plane that hold exact ties
    (feature_cases.tie_depths: S == sigma(p_k) of an early in-box step, where >= / < part company from > / <= and a fused sigma
    would flip the step), frames and counters bit for bit."""
    fused = mode == capi.ARITH_FUSED
    v, tf = phantom(), steep_tf()
    u = uniforms((16, 16, 16))
    far = seeded_depth(u, 2)
    tied, ties = [seeded_depth(u, 8), seeded_depth(u, 9)], 0
    case = fc.Case(W=W, H=H, vec4=v, tf=tf)
    for k, p in enumerate(tied):
        pix, d = fc.tie_depths(case, u, np.random.default_rng(70 + k), count=8000)
        p[pix[:, 1], pix[:, 0]] = d
        ties += len(d)
    assert ties >= 20
    restated = {"far": br.frame(variant, u, W, H, v, tf, None, far, fused=fused),
                "ties": br.frame(variant, u, W, H, v, tf, tied[0], tied[1], fused=fused)}
    assert 0 < restated["ties"][1] < br.frame(variant, u, W, H, v, tf, fused=fused)[1]
    m = br.march(variant, u, W, H, v, tf, None, far)
    ray = m["covered"]
    assert np.all(m["prefix"]) and (m["before_far"][ray] < u.steps_count).sum() * 4 >= ray.sum()
    ctx.set_arithmetic(mode)
    try:
        for fl in (0, 1):
            trivial, (n, cov, _), _, _ = bounded(ctx, bufs, variant, u, v, tf, plane(0.0), plane(1.0), fl)
            cut, (n_cut, _, _), _, _ = bounded(ctx, bufs, variant, u, v, tf, None, far, fl)
            with ob.arithmetic(ob.FUSED if mode == capi.ARITH_FUSED else ob.SEPARATE):
                ref, n_ref, cov_ref = ob.render(variant, u, [v], [tf], W, H, nthreads=4)
                want, total = np.zeros((W * H, 4), f32), 0
                for mm in sorted(set(m["before_far"][ray].tolist())):
                    um = uniforms((16, 16, 16), steps_count=int(mm))
                    sel = np.nonzero(ray & (m["before_far"] == mm))[0]
                    want[sel], k = ob.render_pixels(variant, um, [v], [tf], W, H, m["pixels"][sel], nthreads=4)
                    total += k
            assert np.array_equal(vt.bits(trivial), vt.bits(ref)) and (n, cov) == (n_ref, cov_ref)
            assert np.array_equal(vt.bits(cut.reshape(-1, 4)), vt.bits(want)) and n_cut == total
            assert np.array_equal(vt.bits(cut), vt.bits(restated["far"][0])) and (n_cut, cov) == restated["far"][1:]
            both, (n_both, cov_both, _), _, _ = bounded(ctx, bufs, variant, u, v, tf, tied[0], tied[1], fl)
            print("mode", mode, "variant", variant, "flavour", fl, "ties", ties, "composited", n_both, "restated", restated["ties"][1])
            assert np.array_equal(vt.bits(both), vt.bits(restated["ties"][0])), float(np.nanmax(np.abs(both - restated["ties"][0])))
            assert (n_both, cov_both) == restated["ties"][1:]
    finally:
        ctx.set_arithmetic(capi.ARITH_SEPARATE)


def test_layouts_shapes_and_skipping(ctx, bufs):
    """Layouts 0 / 3 / 1 x flavours 0 / 1 / 6 / 17, synchronous, asynchronous and the tiles of a world of 1 and of 3 give one frame
    per arithmetic mode -- the restatement's in the separately rounded one; on exact-zero air flavour 27 fetches fewer samples than
    it composites, flavour 28 all of them; a table without a zero prefix: 27 runs 28's kernels."""
    v, tf = air_and_core(), steep_tf()
    u = uniforms((24, 24, 24))
    near, far = seeded_depth(u, 8) - f32(0.004), seeded_depth(u, 9)
    ref, n_ref, cov_ref = br.frame(capi.LIGHT, u, W, H, v, tf, near, far)
    assert n_ref > 0
    with capi.Context(W, H, 0) as other:
        try:
            for mode in (capi.ARITH_SEPARATE, capi.ARITH_FUSED):
                ctx.set_arithmetic(mode)
                frames = []
                for layout in (0, 3, 1):
                    ctx.set_volume_layout(layout)
                    for fl in (0, 1, 6, 17):
                        frag, (n, cov, f), ran, _ = bounded(ctx, bufs, capi.LIGHT, u, v, tf, near, far, fl)
                        assert ran == (28 if fl == 1 else 27)
                        assert (n, cov) == (n_ref, cov_ref)
                        assert f < n if fl != 1 else f == n, (layout, fl, f, n)
                        frames.append(frag)
                ctx.set_volume_layout(0)
                bind(ctx, bufs, near, far)
                ctx.render_async(capi.LIGHT, other.frame_device_ptr(), ctx.stream(1))
                assert ctx.counters()[:2] == (n_ref, cov_ref)
                frames.append(other.download()[0])
                for world in (1, 3):
                    full, total = np.zeros((H, W, 4), f32), 0
                    for rank in range(world):
                        cnt = ctx.tile_count(rank, world)
                        ctx.render_tiles(capi.LIGHT, rank, world)
                        total += ctx.counters()[0]
                        if cnt == 0:
                            continue
                        tl = ctx.download_tiles(cnt)[0].reshape(cnt, capi.TILE, capi.TILE, 4)
                        tiles_x = (W + capi.TILE - 1) // capi.TILE
                        for k in range(cnt):
                            ty, tx = divmod(rank + k * world, tiles_x)
                            y0, x0 = ty * capi.TILE, tx * capi.TILE
                            h, w = min(capi.TILE, H - y0), min(capi.TILE, W - x0)
                            full[y0:y0 + h, x0:x0 + w] = tl[k, :h, :w]
                    assert total == n_ref
                    frames.append(full)
                ctx.set_ray_bounds(None, None)
                for fr in frames[1:]:
                    assert np.array_equal(vt.bits(fr), vt.bits(frames[0])), mode
                if mode == capi.ARITH_SEPARATE:
                    assert np.array_equal(vt.bits(frames[0]), vt.bits(ref))
            ctx.set_arithmetic(capi.ARITH_SEPARATE)
            no_prefix = (np.maximum(tf[0], f32(0.01)), tf[1])
            ref2, n2, cov2 = br.frame(capi.LIGHT, u, W, H, v, no_prefix, near, far)
            frag, (n, cov, f), ran, _ = bounded(ctx, bufs, capi.LIGHT, u, v, no_prefix, near, far)
            assert ran == 27 and f == n
            assert np.array_equal(vt.bits(frag), vt.bits(ref2)) and (n, cov) == (n2, cov2)
        finally:
            ctx.set_ray_bounds(None, None)
            ctx.set_arithmetic(capi.ARITH_SEPARATE)
            ctx.set_volume_layout(0)
            ctx.set_kernel_flavour(0)


def test_light_frame_cut_by_the_iso_surface(ctx, bufs):
    """The in-library recipe: an ISO surface frame, its depth computed on the device (vr_surface_depth_async), bound as the far
    bound of a LIGHT frame.  The frame is the restatement's with the downloaded depth; every ISO-hit pixel composites at most the
    ISO march's count for that pixel plus one (per-pixel counts from the restatements, whose frames and totals the GPU's equal)."""
    v, tf = air_and_core(), (hr.default_opacity_tf(64), hr.default_color_tf(64))
    u = uniforms((24, 24, 24))
    ctx.set_iso_value(0.45)
    try:
        ctx.set_output(capi.OUTPUT_SURFACE)
        surf, _, _ = vt.gpu_render(ctx, capi.ISO, u, [v], [tf])
        n_iso = ctx.counters()[0]
        ctx.set_output(capi.OUTPUT_COLOR)
        ctx.surface_depth(ctx.frame_device_ptr(), bufs[1].ptr)
        ctx.set_ray_bounds(None, bufs[1].ptr)
        ctx.render(capi.LIGHT)  # (same stream as the depth pass: ordered behind it)
        frag, _, _ = ctx.download()
        n, cov, _ = ctx.counters()
        assert ctx.last_kernel_flavour() == 27
        depth = bufs[1].read()
    finally:
        ctx.set_output(capi.OUTPUT_COLOR)
        ctx.set_ray_bounds(None, None)
        ctx.set_iso_value(0.5)
    iso = ir.march(u, W, H, v, tf, 0.45)
    assert int(iso["composited"].sum()) == n_iso and iso["hit"].sum() > 50
    assert np.array_equal(vt.bits(depth), vt.bits(sr.depth(surf, u, 0.5)))
    r = br.march(capi.LIGHT, u, W, H, v, tf, None, depth)
    assert np.array_equal(vt.bits(frag.reshape(-1, 4)), vt.bits(r["frag"])) and (n, cov) == (int(r["composited"].sum()), int(r["covered"].sum()))
    hit = iso["hit"]
    assert np.all(r["composited"][hit] <= iso["composited"][hit] + 1)
    free = br.march(capi.LIGHT, u, W, H, v, tf)
    assert r["composited"][hit].sum() < free["composited"][hit].sum()  # (the surface does cut the march)


def test_no_interference(hip):
    """With bounds off, BASIC / LIGHT frames and flavours are what they were before any bounded launch; vr_resize turns the bounds
    off; with bounds on, every other variant, surface output, LIGHT with shadows and both batch entry points return
    VR_ERR_UNSUPPORTED and leave the frame, the counters and the last flavour of the render before them; vr_pick ignores the bounds."""
    vl, tfl = vt.scene(capi.LIGHT, n=16)
    u = uniforms((16, 16, 16))

    def colour(ctx):
        out = []
        for variant in (capi.BASIC, capi.LIGHT):
            out.append((vt.gpu_render(ctx, variant, u, vl, tfl)[0], ctx.counters(), ctx.last_kernel_flavour()))
        return out

    with capi.Context(W, H, 0) as ctx, capi.Context(W, H, 0) as other:
        far = DevBuf(hip, seeded_depth(u, 2))
        try:
            before = colour(ctx)
            assert all(fl not in (27, 28) for _, _, fl in before)
            pick0 = ctx.pick(capi.LIGHT, W // 2, H // 2).as_dict()
            ctx.set_ray_bounds(None, far.ptr)
            cut = vt.gpu_render(ctx, capi.LIGHT, u, vl, tfl)[0]
            assert ctx.last_kernel_flavour() == 27 and not np.array_equal(vt.bits(cut), vt.bits(before[1][0]))
            counters, flavour = ctx.counters(), ctx.last_kernel_flavour()
            pick1 = ctx.pick(capi.LIGHT, W // 2, H // 2).as_dict()
            assert all(np.array_equal(np.asarray(pick0[k]), np.asarray(pick1[k])) for k in pick0)

            def refused(call):
                with pytest.raises(capi.VrError) as e:
                    call()
                assert e.value.code == capi.VR_ERR_UNSUPPORTED
                assert ctx.counters() == counters and ctx.last_kernel_flavour() == flavour
                assert np.array_equal(vt.bits(ctx.download()[0]), vt.bits(cut))

            for variant in (capi.VOLUME_MASK, capi.THREE_FILES, capi.MULTI_CTRT, capi.TF_CALIB, capi.ILLUSTRATIVE, capi.LIGHT_INSHADER,
                            capi.MIP, capi.MINIP, capi.AVERAGE, capi.ISO):
                refused(lambda: ctx.render(variant))
            ctx.set_output(capi.OUTPUT_SURFACE)
            for variant in (capi.BASIC, capi.LIGHT):
                refused(lambda: ctx.render(variant))
            ctx.set_output(capi.OUTPUT_COLOR)
            ctx.set_shadows(2, 1.0)
            refused(lambda: ctx.render(capi.LIGHT))
            ctx.set_shadows(0, 1.0)
            cu = vt.to_capi_uniforms(u)
            refused(lambda: ctx.render_batch_async(capi.LIGHT, [cu], [other.frame_device_ptr()], ctx.stream(0)))
            refused(lambda: ctx.render_tiles_batch_async(capi.LIGHT, 0, 1, [cu, cu], [other.frame_device_ptr()] * 2, ctx.stream(0)))
            # BASIC with shadows on is not LIGHT with shadows on: it runs, bounded
            ctx.set_shadows(2, 1.0)
            vt.gpu_render(ctx, capi.BASIC, u, vl, tfl)
            assert ctx.last_kernel_flavour() == 27
            ctx.set_shadows(0, 1.0)
            ctx.resize(W, H)  # (turns the bounds off)
            after_resize = vt.gpu_render(ctx, capi.LIGHT, u, vl, tfl)[0]
            assert np.array_equal(vt.bits(after_resize), vt.bits(before[1][0])) and ctx.last_kernel_flavour() == before[1][2]
            ctx.set_ray_bounds(None, far.ptr)
            ctx.set_ray_bounds(None, None)
            for a, b in zip(before, colour(ctx)):
                assert np.array_equal(vt.bits(a[0]), vt.bits(b[0])) and a[1][:2] == b[1][:2] and a[2] == b[2]
        finally:
            ctx.set_ray_bounds(None, None)
            far.free()
