"""Seeded random sweep over the five feature marches (csrc/vr_proj.h, vr_iso.h, vr_shadow.h, vr_surf.h, vr_bound.h and the ray
prologue, kernel shell and launcher they share, csrc/vr_ray.h): the cases of feature_cases.py -- non-cubic volumes, ragged viewports,
random cameras, clips, stepping, tables -- x family x arithmetic mode x layout x forced flavour x launch shape (synchronous,
asynchronous into another context's frame, tiles of a world of 1 / 2 / 3, a batch of 2 - 4 cameras), one context per seed resized per
case.  In both arithmetic modes the drawn launch's frame(s) and counters equal the family's float32 restatement bit for bit: the
separately rounded one, or with fused=True the one whose multiply-adds are the ones include/vr.h names under VR_ARITH_FUSED (both are
pinned to the oracle of their mode on the same cases by tests/test_random_features.py, the fused multiply-add itself to exact
arithmetic by tests/test_fma_ref.py).  Fused arithmetic in addition: every form and layout gives one frame -- which is compared with
the restatement too -- and the fused oracle's where it can speak (bounds that cut nothing, the surface alpha plane at the shader's
cut-off, shadows at scale 0, a far bound that leaves the steps 0 .. m-1).  Every case restates its whole frame(s); none is
subsampled.  Fragment modes 1-4 give the oracle's BASIC frame; the flavour, candidate
and fetched invariants of include/vr.h hold; and a plain BASIC / LIGHT frame after a feature launch is the oracle's.  Every message
carries the seed, the case index and the whole draw: feature_cases.cases(seed)[index] replays the case."""
import ctypes as C
import os

import numpy as np
import pytest

import bound_ref as br
import feature_cases as fc
import oracle_binding as ob
import surf_ref as sr
import vrtest as vt
from volumerendering_amd import capi

pytestmark = pytest.mark.gpu
f32 = np.float32
MAX_PIXELS = 149 * 109
FLAVOURS = {"proj": (19, 20), "iso": (21, 22), "shadow": (23, 24), "surf": (25, 26), "bound": (27, 28)}  # (skipping, not)


def _hip():
    try:
        return C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
    except OSError:
        return C.CDLL("libamdhip64.so")  # the runtime libvr_hip.so itself is linked against


class DepthBuf:
    """Device memory for the largest viewport's depth plane, written with synchronous copies (ordered before every later launch)."""

    def __init__(self, hip):
        self.hip, self.p = hip, C.c_void_p()
        assert hip.hipMalloc(C.byref(self.p), C.c_size_t(MAX_PIXELS * 4)) == 0

    def write(self, plane):
        a = np.ascontiguousarray(plane, dtype=f32)
        assert a.size <= MAX_PIXELS
        assert self.hip.hipMemcpy(self.p, a.ctypes.data_as(C.c_void_p), C.c_size_t(a.nbytes), 1) == 0  # hipMemcpyHostToDevice
        return int(self.p.value)

    def free(self):
        if self.p:
            self.hip.hipFree(self.p)
            self.p = C.c_void_p()


def same(a, b):
    """Bit-equal, NaN exactly where the other has NaN."""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    fin = ~np.isnan(b)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(vt.bits(a)[fin], vt.bits(b)[fin])


def assemble(ctx, variant, world, W, H):
    """The frame from the packed tiles of every rank of `world`, and the ranks' counters summed."""
    full, total = np.zeros((H, W, 4), f32), np.zeros(3, np.int64)
    tiles_x = (W + capi.TILE - 1) // capi.TILE
    for rank in range(world):
        cnt = ctx.tile_count(rank, world)
        ctx.render_tiles(variant, rank, world)
        total += np.array(ctx.counters(), np.int64)
        if cnt == 0:
            continue
        tl = ctx.download_tiles(cnt)[0].reshape(cnt, capi.TILE, capi.TILE, 4)
        for k in range(cnt):
            ty, tx = divmod(rank + k * world, tiles_x)
            y0, x0 = ty * capi.TILE, tx * capi.TILE
            h, w = min(capi.TILE, H - y0), min(capi.TILE, W - x0)
            full[y0:y0 + h, x0:x0 + w] = tl[k, :h, :w]
    return full, tuple(int(x) for x in total)


class Sweep:
    """One seed's context, the frames of four more contexts as device memory for the asynchronous shapes, two depth buffers."""

    def __init__(self, hip):
        self.ctx = capi.Context(32, 32, 0)
        self.others = [capi.Context(32, 32, 0) for _ in range(4)]
        self.bufs = [DepthBuf(hip), DepthBuf(hip)]

    def close(self):
        for b in self.bufs:
            b.free()
        for c in self.others + [self.ctx]:
            c.close()

    def feature_on(self, c, family, scale=None, tau=None, near=None, far=None):
        """Switches the family's feature on with the case's parameters (or the pins' overrides); returns the variant to launch."""
        ctx = self.ctx
        if family == "proj":
            return c.proj_variant
        if family == "iso":
            ctx.set_iso_value(c.iso)
            return capi.ISO
        if family == "shadow":
            ctx.set_shadows(c.shadow_divisor, c.shadow_scale if scale is None else scale)
            return capi.LIGHT
        if family == "surf":
            ctx.set_output(capi.OUTPUT_SURFACE)
            ctx.set_surface_threshold(c.tau if tau is None else tau)
            ctx.set_iso_value(c.iso)
            return c.surf_variant
        near, far = (c.near, c.far) if near is None and far is None else (near, far)
        ctx.set_ray_bounds(self.bufs[0].write(near) if near is not None else None, self.bufs[1].write(far) if far is not None else None)
        return c.bound_variant

    def feature_off(self):
        self.ctx.set_output(capi.OUTPUT_COLOR)
        self.ctx.set_shadows(0)
        self.ctx.set_ray_bounds(None, None)

    def sync(self, variant, u):
        """(frame, (composited, covered, fetched), flavour run, candidates) of a synchronous whole-frame launch."""
        ctx = self.ctx
        ctx.set_uniforms(vt.to_capi_uniforms(u))
        ctx.render(variant)
        return ctx.download()[0], ctx.counters(), ctx.last_kernel_flavour(), ctx.kernel_choice()[0]


def expected_flavour(c, family, forced):
    skip, plain = FLAVOURS["iso" if family == "surf" and c.surf_variant == capi.ISO else family]
    return plain if forced == 1 else skip


def draw_launch(g, c):
    """What the GPU side adds to a case: family, arithmetic, layout, forced flavour, launch shape, fragment mode, the leak check."""
    d = dict(family=str(g.choice(fc.FAMILIES)), fused=bool(g.integers(0, 2)), layout=int(g.choice([0, 0, 3, 1])),
             flavour=int(g.choice([0, 1, 6, 17])), shape=str(g.choice(["sync", "async", "tiles", "batch"])),
             stream=int(g.integers(0, 4)), world=int(g.integers(1, 4)), frames=int(g.integers(2, 5)),
             fragment_mode=int(g.integers(1, 5)) if g.random() < 0.15 else 0, leak=int(g.integers(0, 2)) if g.random() < 1 / 3 else None)
    cams = [dict(yaw=float(g.uniform(-3.2, 3.2)), pitch=float(g.uniform(-1.5, 1.5)), distance=float(g.choice([0.5, 0.8, 1.2, 3.0])))
            for _ in range(d["frames"] - 1)]
    d["cameras"] = cams if d["shape"] == "batch" else []  # (drawn in every case: the sequence does not depend on the shape)
    return d


def check_invariants(c, d, counters, ran, cand, what):
    n, cov, f = counters
    assert ran == expected_flavour(c, d["family"], d["flavour"]), ("flavour", ran, what)
    assert cand == [], ("candidates", cand, what)
    assert f <= n and (d["flavour"] != 1 or f == n), ("fetched", counters, what)


def run_case(s, c, d, oracle_mode):
    ctx, family = s.ctx, d["family"]
    W, H, v, tf = c.W, c.H, c.vec4, c.tf
    what = dict(seed=c.seed, index=c.index, draw=c.draw, launch=d)
    fm = d["fragment_mode"]
    us = [c.uniforms(fragment_mode=fm)] + [c.uniforms(fragment_mode=fm, **cam) for cam in d["cameras"]]
    u = us[0]
    ctx.resize(W, H)  # (turns the bounds off)
    for o in s.others:
        o.resize(W, H)
    s.feature_off()
    ctx.set_arithmetic(capi.ARITH_FUSED if d["fused"] else capi.ARITH_SEPARATE)
    ctx.volume_upload(0, v)
    ctx.tf_upload(0, tf[0], tf[1])

    def oracle(variant, uu):
        with ob.arithmetic(oracle_mode):
            return ob.render(variant, uu, [v], [tf], W, H, nthreads=8)

    def want(uu):
        """What frame and (composited, covered) a launch under uu must give; counters None = not defined / not restated."""
        if fm:
            frag, n, cov = oracle(capi.BASIC, uu)
            if family == "surf":  # (BASIC / LIGHT: all counters 0; ISO's are not defined in a fragment mode)
                return frag, (0, 0) if c.surf_variant != capi.ISO else None
            if family in ("shadow", "bound"):  # (the counters are LIGHT's / the variant's: the oracle's in a fragment mode)
                return frag, oracle(capi.LIGHT if family == "shadow" else c.bound_variant, uu)[1:]
            return frag, None
        frag, n, cov = fc.reference(c, family, uu, fused=d["fused"])
        return frag, (n, cov)

    # (a bounded batch is refused: only the first camera is ever rendered)
    rendered = us[:1] if family == "bound" else us
    expect = [want(uu) for uu in rendered]
    # ---- the fused mode: all forms and layouts give one frame, the restatement's, and the fused oracle's where it can speak
    if d["fused"] and not fm:
        variant = s.feature_on(c, family)
        forms = []
        for layout in (0, 3, 1):
            ctx.set_volume_layout(layout)
            for fl in (0, 1, 6, 17):
                ctx.set_kernel_flavour(fl)
                frag, counters, ran, cand = s.sync(variant, u)
                check_invariants(c, dict(d, flavour=fl), counters, ran, cand, ("forms", layout, fl, what))
                forms.append((frag, counters[:2]))
        for frag, nc in forms[1:]:
            assert same(frag, forms[0][0]) and nc == forms[0][1], ("fused forms differ", what)
        assert same(forms[0][0], expect[0][0]), ("fused forms against the fused restatement", forms[0][1], expect[0][1], what)
        assert forms[0][1] == tuple(expect[0][1]), ("fused forms' counters against the fused restatement", forms[0][1], expect[0][1], what)
        ctx.set_volume_layout(0)
        ctx.set_kernel_flavour(0)
        for uu, e in zip(rendered[1:], expect[1:]):
            frag, counters, _, _ = s.sync(variant, uu)
            assert same(frag, e[0]) and counters[:2] == tuple(e[1]), ("fused frame of a batch's camera", counters, e[1], what)
        fused_pins(s, c, d, u, oracle, what)

    # ---- the drawn launch
    ctx.set_volume_layout(d["layout"])
    ctx.set_kernel_flavour(d["flavour"])
    variant = s.feature_on(c, family)
    shape = d["shape"]
    if shape == "batch" and family == "bound":
        frag, counters, ran, cand = s.sync(variant, u)
        check_invariants(c, d, counters, ran, cand, what)
        assert same(frag, expect[0][0]) and counters[:2] == tuple(expect[0][1]), ("bounded frame before the batch", counters, what)
        cus = [vt.to_capi_uniforms(uu) for uu in us]
        ptrs = [o.frame_device_ptr() for o in s.others[:len(us)]]
        for call in (lambda: ctx.render_batch_async(variant, cus, ptrs, ctx.stream(d["stream"])),
                     lambda: ctx.render_tiles_batch_async(variant, 0, 1, cus, ptrs, ctx.stream(d["stream"]))):
            with pytest.raises(capi.VrError) as e:
                call()
            assert e.value.code == capi.VR_ERR_UNSUPPORTED, what
            assert ctx.counters() == counters and ctx.last_kernel_flavour() == ran, ("a refused batch left traces", what)
            assert same(ctx.download()[0], frag), ("a refused batch wrote the frame", what)
    else:
        if shape == "sync":
            frag, counters, ran, cand = s.sync(variant, u)
            got = [frag]
        elif shape == "async":
            ctx.set_uniforms(vt.to_capi_uniforms(u))
            ctx.render_async(variant, s.others[0].frame_device_ptr(), ctx.stream(d["stream"]))
            counters, ran, cand = ctx.counters(), ctx.last_kernel_flavour(), ctx.kernel_choice()[0]
            got = [s.others[0].download()[0]]
        elif shape == "tiles":
            ctx.set_uniforms(vt.to_capi_uniforms(u))
            frag, counters = assemble(ctx, variant, d["world"], W, H)
            ran, cand = ctx.last_kernel_flavour(), ctx.kernel_choice()[0]
            got = [frag]
        else:
            ctx.render_batch_async(variant, [vt.to_capi_uniforms(uu) for uu in us], [o.frame_device_ptr() for o in s.others[:len(us)]],
                                   ctx.stream(d["stream"]))
            counters, ran, cand = ctx.counters(), ctx.last_kernel_flavour(), ctx.kernel_choice()[0]  # (of the last frame)
            got = [o.download()[0] for o in s.others[:len(us)]]
        print(c.seed, c.index, family, shape, "fused" if d["fused"] else "separate", "fragment mode", fm, "counters", counters,
              "expected", expect[len(got) - 1][1], "flavour", ran)
        check_invariants(c, d, counters, ran, cand, what)
        for k, (frag, e) in enumerate(zip(got, expect)):
            assert same(frag, e[0]), ("frame", k, float(np.nanmax(np.abs(np.nan_to_num(frag - e[0])))), what)
        if expect[len(got) - 1][1] is not None:
            assert counters[:2] == tuple(expect[len(got) - 1][1]), ("counters", counters, expect[len(got) - 1][1], what)

    # ---- nothing of the feature stays behind
    if d["leak"] is not None:
        s.feature_off()
        ctx.set_kernel_flavour(0)
        frag, counters, ran, _ = s.sync(d["leak"], u)
        ref, n_ref, cov_ref = oracle(d["leak"], u)
        assert ran not in range(19, 29), ("feature flavour after the feature was switched off", ran, what)
        assert same(frag, ref) and counters[:2] == (n_ref, cov_ref), ("plain frame after a feature launch", d["leak"], counters, what)


def fused_pins(s, c, d, u, oracle, what):
    """Where the fused oracle can speak about the family (the drawn layout and flavour, synchronous)."""
    ctx, family = s.ctx, d["family"]
    W, H, v, tf = c.W, c.H, c.vec4, c.tf
    ctx.set_volume_layout(d["layout"])
    ctx.set_kernel_flavour(d["flavour"])
    if family == "shadow":
        frag, counters, _, _ = s.sync(s.feature_on(c, family, scale=0.0), u)
        ref, n_ref, cov_ref = oracle(capi.LIGHT, u)
        assert same(frag, ref) and counters[:2] == (n_ref, cov_ref), ("fused shadows at scale 0", counters, what)
    elif family == "surf":
        for variant, tau in ((capi.BASIC, sr.TAU_BASIC), (capi.LIGHT, sr.TAU_LIGHT)):
            s.feature_on(c, family, tau=float(tau))
            frag, counters, _, _ = s.sync(variant, u)
            ref, n_ref, _ = oracle(variant, u)
            assert same(frag[..., 3], ref[..., 3]) and counters[0] == n_ref, ("fused surface alpha", variant, counters, what)
            assert counters[1] == int((ref[..., 3] > tau).sum()), ("fused surface hits", variant, counters, what)
    elif family == "bound":
        variant = s.feature_on(c, family, near=np.zeros((H, W), f32), far=np.ones((H, W), f32))
        frag, counters, _, _ = s.sync(variant, u)
        ref, n_ref, cov_ref = oracle(variant, u)
        assert same(frag, ref) and counters[:2] == (n_ref, cov_ref), ("fused bounds near 0 far 1", counters, what)
        if c.near is None and u.toggles[0] == 0 and u.steps_count > 0:
            # a far bound that leaves the steps 0 .. m-1 is the oracle's pixel with steps_count = m (m from the restatement: ray
            # placement, the same in both modes; the variable step would change with steps_count)
            m = br.march(variant, u, W, H, v, tf, None, c.far)
            ray = m["covered"]
            if np.all(m["prefix"]) and ray.any():
                s.feature_on(c, family)
                cut, counters, _, _ = s.sync(variant, u)
                wanted, total = np.zeros((W * H, 4), f32), 0
                for mm in sorted(set(m["before_far"][ray].tolist())):
                    sel = np.nonzero(ray & (m["before_far"] == mm))[0]
                    with ob.arithmetic(ob.FUSED):
                        wanted[sel], k = ob.render_pixels(variant, c.uniforms(steps_count=int(mm)), [v], [tf], W, H, m["pixels"][sel], nthreads=8)
                    total += k
                assert same(cut.reshape(-1, 4), wanted) and counters[0] == total, ("fused far bound as steps_count = m", counters, what)
    s.feature_off()


@pytest.fixture(scope="module")
def hip():
    return _hip()


@pytest.mark.parametrize("seed", fc.SEEDS)
def test_random_feature_launches(hip, seed):
    g = np.random.default_rng(4000 + seed)
    s = Sweep(hip)
    try:
        for c in fc.cases(seed):
            d = draw_launch(g, c)
            run_case(s, c, d, ob.FUSED if d["fused"] else ob.SEPARATE)
    finally:
        s.close()
