"""GPU side of surface extraction (vr_volume_mesh, csrc/vr_mesh.h): positions EQUAL BIT FOR BIT and index arrays EQUAL to the numpy
restatement (mesh_ref.py, pinned on the CPU by tests/test_mesh.py), result and counters as integers -- word and brick edges, boxes inside
and flush, both caps, the settling form against the plain one, flagged bricks, every channel, both layouts, special values, a mesh
behind a signed distance map, the capacities, the errors, no side effects, a random sweep, and the host surface."""
import ctypes as C

import numpy as np
import pytest

import comp_cases as cc
import host_ref as hr
import mesh_cases as mc
import mesh_ref as mr
import outline_ref as orf
import test_components_gpu as tcg
import test_outline_gpu as tog
import vrtest as vt
from volumerendering_amd import capi

pytestmark = pytest.mark.gpu
f32 = np.float32
W, H = 64, 48
EMPTY = (0, 0, 0, 0, (0, 0, 0), (0, 0, 0))


def whole(shape):
    return (0, 0, 0), tuple(shape[::-1])


def desc(shape, level, cap=0, channel=3, box=None, slot=0):
    d = capi.MeshDesc()
    lo, hi = box if box else whole(shape)
    return d.copy(src_slot=slot, channel=channel, level=level, cap=cap, box_lo=lo, box_hi=hi)


def expected_settled(v, level, lo, hi):
    """The voxels of the box that the settling form decides from the range record of their 4^3 brick: the record spans the voxels
    [4 b, min(4 b + 4, n - 1)]^3, is flagged by a NaN, an infinity or a magnitude above 2^125, and settles when max < level or
    min >= level."""
    nz, ny, nx = v.shape
    n = 0
    for bz in range(lo[2] >> 2, (hi[2] + 3) >> 2):
        for by in range(lo[1] >> 2, (hi[1] + 3) >> 2):
            for bx in range(lo[0] >> 2, (hi[0] + 3) >> 2):
                foot = v[4 * bz:min(4 * bz + 4, nz - 1) + 1, 4 * by:min(4 * by + 4, ny - 1) + 1, 4 * bx:min(4 * bx + 4, nx - 1) + 1]
                with np.errstate(invalid="ignore"):
                    if not (np.abs(foot) <= f32(2.0 ** 125)).all():
                        continue
                if foot.max() < f32(level) or foot.min() >= f32(level):
                    n += (max(0, min(hi[0], 4 * bx + 4) - max(lo[0], 4 * bx)) * max(0, min(hi[1], 4 * by + 4) - max(lo[1], 4 * by)) *
                          max(0, min(hi[2], 4 * bz + 4) - max(lo[2], 4 * bz)))
    return n


def check(ctx, d, v, what=None, want=None, settled=None):
    """One vr_volume_mesh against the restatement on component values v (nz, ny, nx): vertices bit for bit, triangles, result, counters.
    settled: the expected out[2] (None: the plain form's 0 unless the call may settle, then 0 <= out[2] <= the box)."""
    verts, tris, res = ctx.volume_mesh(d)
    cnt = ctx.mesh_counters()
    want = want or mr.extract(v, d.level, d.cap, tuple(d.box_lo), tuple(d.box_hi))
    assert res.as_tuple() == want["result"], (what, res.as_tuple(), want["result"])
    assert verts.shape == want["vertices"].shape and tris.shape == want["triangles"].shape, what
    bad = np.argwhere(vt.bits(verts) != vt.bits(want["vertices"]))
    assert bad.size == 0, (what, len(bad), bad[:4], verts[bad[:4, 0]], want["vertices"][bad[:4, 0]])
    bad = np.argwhere(tris != want["triangles"])
    assert bad.size == 0, (what, len(bad), bad[:4])
    box = int(np.prod([max(0, b - a) for a, b in zip(d.box_lo, d.box_hi)]))
    assert cnt[0] == box and cnt[1] + cnt[2] == box and cnt[3] == want["result"][3], (what, cnt, box)
    if settled is not None:
        assert cnt[2] == settled, (what, cnt, settled)
    if d.cap:
        assert mr.is_closed(tris), what
    return verts, tris, res, cnt, want


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


@pytest.mark.parametrize("nx", [63, 64, 65, 129])
def test_word_and_brick_edges(ctx, nx):
    """Rows of 63, 64, 65 and 129 points (with the cap: 65, 66, 67, 131), sizes that are no multiple of the brick, a box flush with the
    volume and one strictly inside it, both caps, the settling form and the plain one."""
    shape = (6, 7, nx)
    v = mc.smooth_noise(shape, seed=nx)
    ctx.volume_upload(0, mc.vec4(v, 3, seed=1))
    inner = ((1, 2, 1), (nx - 1, 6, 5))
    for box in (None, inner):
        for cap in (0, 1):
            d = desc(shape, 0.1, cap, box=box)
            want = mr.extract(v, d.level, cap, tuple(d.box_lo), tuple(d.box_hi))
            assert want["result"][1] > 100
            for flavour in (0, 1):
                ctx.set_kernel_flavour(flavour)
                check(ctx, d, v, (nx, box, cap, flavour), want, settled=0 if flavour else expected_settled(v, 0.1, d.box_lo, d.box_hi))


def test_settling_against_the_plain_form(ctx):
    """Constant bricks settle (out[2] > 0, nothing loaded there) and give the same bits as the plain form; a brick with a NaN voxel is
    flagged and not settled; an infinity flags as well."""
    shape = (13, 18, 22)
    v = np.zeros(shape, f32)
    v[2:11, 3:15, 5:19] = 1
    v[5, 8, 9] = 0.25
    vols = {"plain": v.copy(), "nan": v.copy(), "inf": v.copy()}
    vols["nan"][1, 1, 1] = np.nan     # in a brick of zeros: out, and its brick is loaded
    vols["nan"][6, 9, 12] = np.nan    # in a brick of ones: out, a hole
    vols["inf"][6, 9, 12] = np.inf    # inside, flagged
    vols["inf"][12, 17, 21] = -np.inf
    settled = {}
    for name, vol in vols.items():
        ctx.volume_upload(0, mc.vec4(vol, 3, seed=2))
        for box in (None, ((2, 1, 0), (21, 17, 12))):
            for cap in (0, 1):
                d = desc(shape, 0.5, cap, box=box)
                want = mr.extract(vol, 0.5, cap, tuple(d.box_lo), tuple(d.box_hi))
                ctx.set_kernel_flavour(0)
                n = expected_settled(vol, 0.5, d.box_lo, d.box_hi)
                check(ctx, d, vol, (name, box, cap, 0), want, settled=n)
                ctx.set_kernel_flavour(1)
                check(ctx, d, vol, (name, box, cap, 1), want, settled=0)
                settled[name, box is None] = n
    assert 0 < settled["nan", True] < settled["plain", True] and 0 < settled["inf", True] < settled["plain", True]


def test_a_brick_of_ones_at_the_box_face(ctx):
    """A 5 x 5 x 5 box of ones is what one brick's cells touch: with cap = 0 everything settles and nothing is emitted; with cap = 1 the
    same voxels settle and the cap is emitted all the same -- a closed box of volume 64."""
    v = np.ones((5, 5, 5), f32)
    ctx.volume_upload(0, mc.vec4(v, 3, seed=3))
    _, _, res, cnt, _ = check(ctx, desc(v.shape, 0.5, 0), v, "open", settled=125)
    assert res.as_tuple() == (0, 0, 125, 0, (0, 0, 0), (0, 0, 0)) and cnt == (125, 0, 125, 0)
    verts, tris, res, cnt, _ = check(ctx, desc(v.shape, 0.5, 1), v, "capped", settled=125)
    assert res.n_triangles > 0 and cnt[1] == 0 and mr.signed_volume(verts, tris) == 64.0 and mr.euler(len(verts), tris) == 2
    assert (res.as_tuple()[4], res.as_tuple()[5]) == ((-1, -1, -1), (5, 5, 5))


@pytest.mark.parametrize("layout", [0, 3])
def test_channels_and_layouts(ctx, layout):
    """Channels 0 .. 2 have no records and take the plain form; channel 3 settles; the same bits in both volume layouts."""
    shape = (9, 14, 21)
    ctx.set_volume_layout(layout)
    vol = np.stack([mc.smooth_noise(shape, seed=10 + k) for k in range(4)], axis=-1)
    vol[2:8, 4:12, 4:16, 3] = 2.0
    ctx.volume_upload(1, vol)
    for k in range(4):
        for cap in (0, 1):
            d = desc(shape, 0.2, cap, channel=k, slot=1, box=((1, 0, 0), (21, 13, 9)))
            v = np.ascontiguousarray(vol[..., k])
            _, _, res, cnt, _ = check(ctx, d, v, (layout, k, cap), settled=expected_settled(v, 0.2, d.box_lo, d.box_hi) if k == 3 else 0)
            assert res.n_triangles > 0 and (cnt[2] > 0) == (k == 3)


def test_values(ctx):
    """The level equal to voxel values, +-inf, NaN, -0.0f, and a mask of 0 / 1 at level 0.5."""
    rng = np.random.default_rng(5)
    shape = (7, 9, 11)
    v = rng.integers(-2, 3, size=shape).astype(f32)
    v[rng.random(shape) < 0.08] = np.inf
    v[rng.random(shape) < 0.08] = -np.inf
    v[rng.random(shape) < 0.08] = np.nan
    v[rng.random(shape) < 0.08] = -0.0
    ctx.volume_upload(0, mc.vec4(v, 3, seed=6))
    for level in (0.0, -0.0, 1.0, -2.0, 2.0, 0.5, 1e-45, 3.0e38):
        for cap in (0, 1):
            for flavour in (0, 1):
                ctx.set_kernel_flavour(flavour)
                verts, _, _, _, _ = check(ctx, desc(shape, level, cap), v, (level, cap, flavour))
                assert np.isfinite(verts).all()
    m = mc.random_mask()
    ctx.volume_upload(0, mc.vec4(m, 2, seed=7))
    _, tris, res, _, _ = check(ctx, desc(m.shape, 0.5, 1, channel=2), m, "mask")
    assert res.as_tuple()[:2] == (1648, 3420)


def test_composition_with_a_signed_distance_map(ctx):
    """vr_mask_distance SIGNED into a channel, then the mesh at level 0 of that channel equals the restatement on the downloaded channel."""
    shape = (12, 17, 23)
    z, y, x = mc.grid(shape)
    m = np.zeros(shape + (4,), f32)
    m[..., 0] = (x * x / 60.0 + y * y / 30.0 + z * z / 16.0) < 1.0
    ctx.volume_upload(0, m)
    ctx.volume_upload(1, np.zeros(shape + (4,), f32))
    ctx.mask_distance(ctx.dist_whole(0, 0, 1, 2, capi.DIST_SIGNED))
    field = np.ascontiguousarray(ctx.volume_download(1, shape)[..., 2])
    assert (field < 0).any() and (field > 0).any()
    for level, cap in ((0.0, 0), (0.0, 1), (-1.5, 1), (1.5, 0)):
        verts, tris, res, _, _ = check(ctx, desc(shape, level, cap, channel=2, slot=1), field, (level, cap))
        assert res.n_triangles > 200


def raw(ctx, d, n_vertices, n_triangles, sentinel=0x5A):
    """One raw vr_volume_mesh with buffers of the given capacities, pre-filled with a sentinel: (rc, vertices, triangles, result)."""
    verts = np.frombuffer(bytes([sentinel]) * (max(n_vertices, 1) * 12), np.uint32).copy().reshape(-1, 3)
    tris = np.frombuffer(bytes([sentinel]) * (max(n_triangles, 1) * 12), np.uint32).copy().reshape(-1, 3)
    full = d.copy(max_vertices=n_vertices, max_triangles=n_triangles, vertices=verts.ctypes.data if n_vertices else None,
                  triangles=tris.ctypes.data if n_triangles else None)
    res = capi.MeshResult()
    rc = ctx.lib.vr_volume_mesh(ctx.h, C.byref(full), C.byref(res))
    return rc, verts, tris, res


def test_capacity(ctx):
    shape = (8, 11, 14)
    v = mc.smooth_noise(shape, seed=21)
    ctx.volume_upload(0, mc.vec4(v, 3, seed=22))
    d = desc(shape, 0.0, 1)
    want = mr.extract(v, 0.0, 1, *whole(shape))
    n, q = want["result"][:2]
    s = 0x5A5A5A5A
    assert n > 50 and q > 50
    rc, verts, tris, res = raw(ctx, d, 0, 0)  # the counting call
    assert rc == capi.VR_OK and res.as_tuple() == want["result"] and ctx.mesh_counters()[3] == want["result"][3]
    rc, verts, tris, res = raw(ctx, d, n, q)  # exact capacity
    assert rc == capi.VR_OK and res.as_tuple() == want["result"]
    assert np.array_equal(verts, vt.bits(want["vertices"])) and np.array_equal(tris, want["triangles"])
    rc, verts, tris, res = raw(ctx, d, n + 7, q + 3)  # more than needed: the rest keeps the sentinel
    assert rc == capi.VR_OK and np.array_equal(verts[:n], vt.bits(want["vertices"])) and (verts[n:] == s).all()
    assert np.array_equal(tris[:q], want["triangles"]) and (tris[q:] == s).all()
    for cap in ((n - 1, q), (n, q - 1), (0, q), (n, 0), (1, 1)):  # one vertex short, one triangle short, one buffer missing
        rc, verts, tris, res = raw(ctx, d, *cap)
        assert rc == capi.VR_ERR_INVALID_ARG, cap
        err = ctx.lib.vr_last_error(ctx.h).decode()
        assert err.startswith("vr_volume_mesh") and str(n) in err and str(q) in err, err
        assert (verts == s).all() and (tris == s).all(), cap
        assert res.as_tuple() == want["result"], cap
    check(ctx, d, v, want=want)  # (the context is usable)


def ended(ctx, began, what):
    """vr_mesh_timing after a call that began `began` phases: those are timed, the later ones exactly 0.0."""
    ms = ctx.mesh_timing()
    assert all(t > 0.0 for t in ms[:began]) and ms[began:] == (0.0,) * (4 - began), (what, ms)


def test_argument_errors_leave_the_context_usable(ctx):
    """... and what vr_mesh_timing and vr_mesh_counters report after each ending a small input reaches: a phase the call never began
    is exactly 0.0, the counters are the call's own, and an argument error leaves both as they were."""
    shape = (5, 12, 30)
    nz, ny, nx = shape
    v = mc.smooth_noise(shape, seed=31)
    ctx.volume_upload(0, mc.vec4(v, 3, seed=32))
    good = desc(shape, 0.0, 1)
    _, _, res, _, _ = check(ctx, good, v)
    ended(ctx, 4, "full call")
    counters, timing = ctx.mesh_counters(), ctx.mesh_timing()
    verts = np.zeros((4, 3), f32)
    tris = np.zeros((4, 3), np.uint32)
    invalid = [dict(src_slot=-1), dict(src_slot=3), dict(channel=-1), dict(channel=4), dict(level=np.nan), dict(level=np.inf), dict(level=-np.inf),
               dict(cap=-1), dict(cap=2), dict(box_lo=(-1, 0, 0)), dict(box_hi=(nx + 1, ny, nz)), dict(box_hi=(nx, ny, nz + 1)),
               dict(box_lo=(5, 0, 0), box_hi=(4, ny, nz)), dict(max_vertices=4), dict(max_triangles=4), dict(vertices=verts.ctypes.data),
               dict(triangles=tris.ctypes.data)]
    for over in invalid:
        d = good.copy(**over)
        assert ctx.lib.vr_volume_mesh(ctx.h, C.byref(d), C.byref(capi.MeshResult())) == capi.VR_ERR_INVALID_ARG, over
        assert (ctx.lib.vr_last_error(ctx.h) or b"").decode().startswith("vr_volume_mesh"), over
    assert ctx.lib.vr_volume_mesh(ctx.h, None, None) == capi.VR_ERR_INVALID_ARG
    assert ctx.lib.vr_volume_mesh(None, C.byref(good), None) == capi.VR_ERR_INVALID_ARG
    assert ctx.lib.vr_mesh_counters(ctx.h, None) == capi.VR_ERR_INVALID_ARG
    assert ctx.lib.vr_mesh_timing(ctx.h, None) == capi.VR_ERR_INVALID_ARG
    assert ctx.mesh_counters() == counters and ctx.mesh_timing() == timing
    # the counting call and a buffer one element short end behind the counts; both report their own counters
    part = desc(shape, 0.0, 1, box=((2, 1, 1), (nx, ny - 2, 3)))
    n2, q2 = mr.extract(v, 0.0, 1, tuple(part.box_lo), tuple(part.box_hi))["result"][:2]
    assert 0 < n2 < res.n_vertices
    for d, caps, rc in ((part, (0, 0), capi.VR_OK), (good, (res.n_vertices - 1, res.n_triangles), capi.VR_ERR_INVALID_ARG),
                        (part, (n2, q2 - 1), capi.VR_ERR_INVALID_ARG)):
        assert raw(ctx, d, *caps)[0] == rc, caps
        ended(ctx, 2, caps)
        assert ctx.mesh_counters()[0] == (nx * ny * nz if d is good else (nx - 2) * (ny - 3) * 2), caps
        before = ctx.mesh_counters(), ctx.mesh_timing()
        assert raw(ctx, d.copy(cap=2), *caps)[0] == capi.VR_ERR_INVALID_ARG
        assert (ctx.mesh_counters(), ctx.mesh_timing()) == before, caps
    assert raw(ctx, good, res.n_vertices, res.n_triangles)[0] == capi.VR_OK  # exact capacity
    ended(ctx, 4, "exact capacity")
    assert ctx.mesh_counters() == counters
    with capi.Context(W, H, 0) as empty:
        assert empty.lib.vr_volume_mesh(empty.h, C.byref(good), None) == capi.VR_ERR_NOT_READY
        err = empty.lib.vr_last_error(empty.h)
        assert err.startswith(b"vr_volume_mesh") and b"empty" in err
        assert empty.lib.vr_mesh_whole(empty.h, 0, C.byref(capi.MeshDesc())) == capi.VR_ERR_NOT_READY
    # vr_mesh_whole
    assert bytes(ctx.mesh_whole(0)) == bytes(desc(shape, 0.5, 0))
    for bad in (3, -1):
        assert ctx.lib.vr_mesh_whole(ctx.h, bad, C.byref(capi.MeshDesc())) == capi.VR_ERR_INVALID_ARG
    assert ctx.lib.vr_mesh_whole(ctx.h, 0, None) == capi.VR_ERR_INVALID_ARG
    # a NULL result is fine; an empty box, a box without cells and a level nothing reaches give no triangles
    assert ctx.lib.vr_volume_mesh(ctx.h, C.byref(good), None) == capi.VR_OK
    for box, cap in ((((3, 2, 1), (3, 9, 3)), 1), (((0, 0, 2), (nx, ny, 2)), 0)):
        _, _, res, cnt, _ = check(ctx, desc(shape, 0.0, cap, box=box), v, box)
        assert res.as_tuple() == EMPTY and cnt == (0, 0, 0, 0)
        ended(ctx, 0, box)
        assert raw(ctx, good.copy(channel=4), 0, 0)[0] == capi.VR_ERR_INVALID_ARG
        assert ctx.mesh_counters() == (0, 0, 0, 0) and ctx.mesh_timing() == (0.0,) * 4
    _, _, res, cnt, _ = check(ctx, desc(shape, 0.0, 0, box=((0, 3, 0), (nx, 4, nz))), v, "one row thick")
    assert res.as_tuple()[:2] == (0, 0) and res.inside > 0 and cnt[0] == nx * nz
    _, _, res, cnt, _ = check(ctx, desc(shape, 0.0, 1, box=((0, 3, 0), (nx, 4, nz))), v, "one row thick, capped")
    assert res.n_triangles > 0
    _, _, res, cnt, _ = check(ctx, desc(shape, 1e30, 1), v, "nothing inside")
    assert res.as_tuple() == EMPTY and cnt[0] == nx * ny * nz
    ended(ctx, 2, "nothing inside")
    assert raw(ctx, desc(shape, 1e30, 1), 4, 4)[0] == capi.VR_OK  # (no crossing edge: nothing to emit into the buffers either)
    ended(ctx, 2, "nothing inside, with buffers")


def test_side_effects():
    """The call writes no slot and disturbs nothing: the slots' bits, a rendered frame, vr_last_counters and what the other tools report
    are the same before and after."""
    n = 16
    variant = capi.VOLUME_MASK
    vols, tfs = vt.scene(variant, n)
    step, count = hr.stepping_params(n, n, n)
    u = hr.make_uniforms(W, H, steps_count=count, step_size=step)
    with capi.Context(W, H, 0) as c:
        frame, _, _ = vt.gpu_render(c, variant, u, vols, tfs)
        c.mask_morph(c.morph_whole(0, 0, 0, 1, capi.MORPH_DILATE))
        c.mask_outlines(c.outlines_whole(0))
        c.render(variant)
        frame = c.download()[0]

        def reports():
            return (c.counters(), c.last_kernel_flavour(), len(c.kernel_times()), c.grow_counters(), c.grow_timing(), c.morph_counters(),
                    c.morph_timing(), c.dist_counters(), c.dist_timing(), c.polygons_counters(), c.polygons_timing(), c.outlines_counters(),
                    c.outlines_timing())

        earlier = reports()
        before = [c.volume_download(s, vols[s].shape[:3]) for s in range(len(vols))]
        assert c.mesh_counters() == (0, 0, 0, 0) and c.mesh_timing() == (0.0, 0.0, 0.0, 0.0)
        slot, k = next((s, k) for s in range(len(vols)) for k in (3, 0) if before[s][..., k].min() < before[s][..., k].max())
        v = np.ascontiguousarray(before[slot][..., k])
        level = float(f32(0.5) * (v.min() + v.max()))
        _, _, res, cnt, _ = check(c, c.mesh_whole(slot).copy(channel=k, level=level, cap=1), v)
        assert res.n_triangles > 0 and cnt[3] > 0
        timing = c.mesh_timing()
        assert len(timing) == 4 and all(t > 0.0 for t in timing)
        assert reports() == earlier
        for s in range(len(vols)):
            assert np.array_equal(vt.bits(c.volume_download(s, vols[s].shape[:3])), vt.bits(before[s]))
        assert np.array_equal(vt.bits(c.download()[0]), vt.bits(frame))
        c.render(variant)
        assert np.array_equal(vt.bits(c.download()[0]), vt.bits(frame))
        assert (c.counters(), c.last_kernel_flavour()) == earlier[:2]


def test_one_scan_buffer_serves_three_tools(ctx):
    """Contour tracing, connected components and surface extraction take the tile sums of their scans from one buffer of the context.
    Two volumes, (60, 36, 4) voxels -- 2160 words of one voxel row each, three scan tiles, in every tool -- and (4, 6, 10); the tools
    run in turn on the small and the large one, each behind each of the others, and every output equals its restatement: a scan that
    read the tile sums another call left behind fails here."""
    calls = {}
    for slot, shape in enumerate(((60, 36, 4), (4, 6, 10))):
        nz, ny, nx = shape
        z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
        ball = (f32(0.4) * max(shape) - np.sqrt((x - 0.5 * nx) ** 2 + (y - 0.45 * ny) ** 2 + (z - 0.5 * nz) ** 2)).astype(f32)
        state = mc.vec4(ball, 3, seed=75 + slot)
        state[..., 0] = cc.random_set(shape, 0.5, 71 + slot)
        ctx.volume_upload(slot, state)
        m = orf.members(state)
        o, k, s = tog.desc(shape, src_slot=slot), tcg.desc(shape, src_slot=slot), desc(shape, 0.0, slot=slot)
        wo, wk, ws = tog.reference(o, m), tcg.reference(k, state, None), mr.extract(ball, 0.0, 0, *whole(shape))
        calls["o", slot] = lambda o=o, m=m, wo=wo: tog.check(ctx, o, m, want=wo)
        calls["k", slot] = lambda k=k, state=state, wk=wk: tcg.check(ctx, k, state, want=wk)
        calls["s", slot] = lambda s=s, ball=ball, ws=ws: check(ctx, s, ball, want=ws)
        if slot == 0:  # (not vacuous: the scans over the words, the corners and the runs chain over several tiles; there is a surface)
            assert nz * ny > 2 * 1024 and wo["result"][0] > 2 * 1024 and wk["counters"][1] > 2 * 1024 and ws["result"][0] > 100
    order = "oksoskok"  # every tool behind each of the others
    assert {a + b for a, b in zip(order, order[1:])} >= {"ok", "os", "ko", "ks", "so", "sk"}
    for first in (1, 0):  # small, large, small, ..; then large, small, large, ..: every tool meets both sizes behind every other
        for i, tool in enumerate(order):
            calls[tool, (first + i) % 2]()


SWEEP = mc.sweep(40)


@pytest.mark.parametrize("i", range(40))
def test_random_sweep(ctx, i):
    case = SWEEP[i]
    ctx.set_kernel_flavour(1 if case["plain"] else 0)
    ctx.volume_upload(i % 3, mc.vec4(case["v"], case["channel"], seed=case["seed"]))
    d = capi.MeshDesc().copy(src_slot=i % 3, channel=case["channel"], level=case["level"], cap=case["cap"], box_lo=case["box_lo"], box_hi=case["box_hi"])
    settles = case["channel"] == 3 and not case["plain"]
    check(ctx, d, case["v"], i, settled=expected_settled(case["v"], case["level"], case["box_lo"], case["box_hi"]) if settles else 0)


def test_application_extract_surface(tmp_path):
    """Application::ExtractSurface + WriteStl / WritePly, read back with numpy: the triangle count, the positions scaled by the spacing in
    float64, the facet normals."""
    from volumerendering_amd import host
    shape = (9, 12, 15)
    v = mc.smooth_noise(shape, seed=41)
    vol = mc.vec4(v, 3, seed=42)
    spacing = (0.977, 0.977, 2.5)
    want = mr.extract(v, 0.1, 1, *whole(shape))
    n, q = want["result"][:2]
    pos = want["vertices"].astype(np.float64) * np.array(spacing)
    with host.Application(W, H, 0) as app:
        app.OnStart(capi.BASIC, [host.VolumeFile.from_vec4(vol)])
        app.context().volume_upload(1, vol)
        mesh = app.extract_surface(1, 3, 0.1, 1, spacing=spacing)
        assert mesh.result.as_tuple() == want["result"]
        assert np.array_equal(mesh.positions, pos) and np.array_equal(mesh.triangles, want["triangles"])
        unit = app.extract_surface(1, 3, 0.1, 1)
        assert np.array_equal(unit.positions, want["vertices"].astype(np.float64))
        mesh.write_stl(tmp_path / "s.stl")
        mesh.write_ply(tmp_path / "s.ply")
    # STL: 80 bytes, the count, 50 bytes a triangle
    blob = (tmp_path / "s.stl").read_bytes()
    assert len(blob) == 84 + 50 * q and int(np.frombuffer(blob, np.uint32, 1, 80)[0]) == q
    rec = np.frombuffer(blob, np.dtype([("n", "<f4", 3), ("p", "<f4", (3, 3)), ("a", "<u2")]), q, 84)
    corners = pos[want["triangles"].astype(np.int64)]
    assert np.array_equal(rec["p"], corners.astype(f32)) and (rec["a"] == 0).all()
    nrm = np.cross(corners[:, 1] - corners[:, 0], corners[:, 2] - corners[:, 0])
    ln = np.linalg.norm(nrm, axis=1)
    ok = ln > 0
    assert np.allclose(rec["n"][ok], nrm[ok] / ln[ok, None], atol=1e-6) and (rec["n"][~ok] == 0).all()
    # PLY: the header, float32 vertices, 13 bytes a face
    blob = (tmp_path / "s.ply").read_bytes()
    head, body = blob.split(b"end_header\n", 1)
    assert head.startswith(b"ply\nformat binary_little_endian 1.0\n") and f"element vertex {n}\n".encode() in head and f"element face {q}\n".encode() in head
    assert len(body) == 12 * n + 13 * q
    assert np.array_equal(np.frombuffer(body, "<f4", 3 * n).reshape(-1, 3), pos.astype(f32))
    faces = np.frombuffer(body, np.dtype([("k", "u1"), ("i", "<u4", 3)]), q, 12 * n)
    assert (faces["k"] == 3).all() and np.array_equal(faces["i"], want["triangles"])
