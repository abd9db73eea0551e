"""The gamma index on the device (vr_volume_gamma, include/vr.h) against the numpy restatement (gamma_ref.py): the downloaded destination
slot, the result struct, all three counters and the untouched dose slots, BIT FOR BIT with no NaN escape, in both kernel forms
(flavour 0: LDS tiles and the exact cut; flavour 1: plain, every candidate) and in the volume layouts 0, 1 and 3.

The default form's tile (csrc/vr_gamma.h) is 32 outputs along x, 8 along y and 4 along z; the volumes of 37 x 21 x 13 voxels hold two
tiles and a tail along x, three along y and four along z.  The cases of gamma_cases.py go to the tile's, the index range's and the
cut's edges."""
import ctypes as C

import numpy as np
import pytest

import gamma_cases as gc
import gamma_ref as gr
import host_ref as hr
import index_edges_cases as ie
import oracle_binding as ob
import resample_cases as rc
import vrtest as vt
from volumerendering_amd import capi

pytestmark = pytest.mark.gpu
f32, u32 = np.float32, np.uint32
W, H = 64, 48
FORMS = [(0, 0), (1, 0), (0, 1), (1, 1), (0, 3), (1, 3)]  # (flavour, layout)
SHAPE = (13, 21, 37)  # (nz, ny, nx)
S = (1000, 1000, 3000)  # 1 x 1 x 3 mm in micrometres
GLOBAL, LOCAL, QNAN = capi.GAMMA_GLOBAL, capi.GAMMA_LOCAL, gr.QNAN
PAYLOAD = gc.PAYLOAD  # a signalling NaN with a payload


doses = gc.doses


def describe(ctx, slots, chans, p):
    d = ctx.gamma_whole(slots[0], chans[0], slots[1], chans[1], slots[2], chans[2])
    return d.copy(spacing=p["spacing"], dta=p["dta"], reach=p["reach"], sub=p["sub"], mode=p["mode"], dose_tolerance=p["tol"], cutoff=p["cutoff"],
                  skip_bits=p["skip_bits"], roi_slot=p["roi"][0], roi_contour=p["roi"][1], box_lo=p["lo"], box_hi=p["hi"])


def check(ctx, ref, ev, before, spacing=S, dta=3000, reach=3000, sub=1, mode=GLOBAL, tol=0.6, cutoff=-np.inf, skip_bits=QNAN, roi=(-1, 0),
          box=None, chans=(3, 3, 0), slots=(0, 1, 2), forms=FORMS[:2], what=None, extra=None):
    """One descriptor in every form against the restatement.  ref, ev: the voxels of slots[0] and slots[1] (one array when they are one
    slot); before: the voxels of slots[2] before the call (ignored where it is a dose's slot; None: the slot is empty and the call
    creates it -- one form only).  roi: (slot, contour), the slot one of the three or one of extra = {slot: voxels}.  Every slot is
    uploaded again for every form.  Returns the restatement's (volume, result, counters)."""
    shape = ref.shape[:3]
    lo, hi = box if box else ((0, 0, 0), rc.n_of(shape))
    vols = dict(extra or {})
    vols[slots[2]] = before
    vols[slots[1]] = ev
    vols[slots[0]] = ref
    p = dict(spacing=spacing, dta=dta, reach=reach, sub=sub, mode=mode, tol=tol, cutoff=cutoff, skip_bits=skip_bits, roi=roi, lo=lo, hi=hi)
    want, want_res, want_cnt = gr.gamma(vols[slots[0]], vols[slots[1]], vols[slots[2]], chans[0], chans[1], chans[2], spacing, dta, reach, sub, mode,
                                        tol, cutoff, skip_bits, None if roi[0] < 0 else vols[roi[0]], roi[1], lo, hi)
    for flavour, layout in forms:
        ctx.set_kernel_flavour(flavour)
        ctx.set_volume_layout(layout)
        for slot, v in vols.items():
            if v is not None:
                ctx.volume_upload(slot, v)
        res = ctx.volume_gamma(describe(ctx, slots, chans, p))
        cnt = ctx.gamma_counters()
        got = ctx.volume_download(slots[2], shape)
        if not np.array_equal(vt.bits(got), vt.bits(want)):
            bad = np.argwhere(vt.bits(got) != vt.bits(want))
            raise AssertionError((what, flavour, layout, len(bad), bad[:4], hex(vt.bits(got)[tuple(bad[0])]), hex(vt.bits(want)[tuple(bad[0])])))
        assert res.as_tuple() == want_res, (what, flavour, layout, res.as_tuple(), want_res)
        assert cnt == want_cnt, (what, flavour, layout, cnt, want_cnt)
        for slot, v in vols.items():
            if slot != slots[2]:
                assert np.array_equal(vt.bits(ctx.volume_download(slot, shape)), vt.bits(v)), (what, flavour, layout, slot)
    return want, want_res, want_cnt


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


@pytest.fixture(scope="module")
def pair():
    return doses(SHAPE, 11)


@pytest.fixture(scope="module")
def before():
    return rc.arbitrary_bits(SHAPE, 12)


def test_forms_and_layouts(ctx, pair, before):
    """Both kernel forms in the layouts 0, 1 and 3: 3 % / 3 mm at 1 x 1 x 3 mm with the reach of 6 mm (293 offsets) over the whole volume,
    into a destination of arbitrary bits whose other three components keep theirs."""
    _, res, cnt = check(ctx, *pair, before, reach=6000, forms=FORMS, what="forms")
    assert cnt == (37 * 21 * 13, 37 * 21 * 13, 293) and 0 < res[2] < res[1] and res[3] == 0


def test_a_box_off_the_tile_origin(ctx, pair, before):
    """A box that starts at (3, 2, 1) and ends inside a tile on every axis: 33 x 11 x 6 outputs; the outside of the box keeps its bits."""
    want, res, _ = check(ctx, *pair, before, reach=6000, sub=2, box=((3, 2, 1), (36, 13, 7)), chans=(3, 3, 2), what="box")
    assert res[0] == 33 * 11 * 6
    keep = np.ones(SHAPE, bool)
    keep[1:7, 2:13, 3:36] = False
    assert np.array_equal(vt.bits(want)[keep], vt.bits(before)[keep])


FACES = [((0, 8, 5), (2, 12, 8)), ((35, 8, 5), (37, 12, 8)), ((15, 0, 5), (19, 2, 8)), ((15, 19, 5), (19, 21, 8)), ((15, 8, 0), (19, 12, 2)),
         ((15, 8, 11), (19, 12, 13))]


@pytest.mark.parametrize("k", range(6), ids=["x0", "x1", "y0", "y1", "z0", "z1"])
def test_a_window_crossing_each_face(ctx, pair, before, k):
    """A thin box at each of the six faces with a reach of two voxels on every axis: the positions beyond the face are no candidates, at
    sub 1 and, with the upper corners of the interpolation, at sub 2."""
    for sub in (1, 2):
        check(ctx, *pair, before, spacing=(1000, 1000, 1000), dta=2000, reach=2000, sub=sub, box=FACES[k], what=(k, sub))


def test_a_z_radius_of_zero(ctx, pair, before):
    """Spacing (1000, 1000, 3000) with reach 2000: no offset leaves the slice (13 offsets), the tile has no halo along z."""
    _, _, cnt = check(ctx, *pair, before, reach=2000, forms=FORMS[:2] + FORMS[4:5], what="z radius 0")
    assert cnt[2] == 13


def test_reach_below_the_spacing(ctx, pair, before):
    """sub 1: K = 1 and gamma = |E - R| / T (the square root of d * d, d = (e - r) * invT).  sub 2: nine offsets, those with f_a > 0 need
    b_a + 1 and vanish at the upper faces, where the last voxel keeps the offsets with f_a == 0 alone."""
    ref, ev = pair
    want, _, cnt = check(ctx, ref, ev, before, reach=900, tol=0.5, what="K = 1")
    assert cnt[2] == 1
    d = (ev[..., 3] - ref[..., 3]) * (f32(1.0) / f32(0.5))
    assert np.array_equal(vt.bits(want[..., 0]), vt.bits(np.sqrt(d * d)))  # (d * d is exact to f32 here or not: the same single rounding)
    _, _, cnt = check(ctx, ref, ev, before, reach=900, sub=2, what="K = 9")
    assert cnt[2] == 9
    check(ctx, ref, ev, before, reach=900, sub=2, box=((30, 15, 9), (37, 21, 13)), what="K = 9, upper corner")


@pytest.mark.parametrize("sub", [1, 2, 3, 4])
def test_sub(ctx, pair, before, sub):
    """1 to 4 candidate positions per voxel step, reach 1.5 voxels in the slice: the interpolation along x, then y, then z."""
    check(ctx, *pair, before, dta=1000, reach=1500, sub=sub, forms=FORMS[:2] + FORMS[4:], what=sub)
    check(ctx, *pair, before, spacing=(1000, 1000, 1000), dta=1000, reach=1000, sub=sub, box=((20, 10, 6), (37, 21, 13)), what=(sub, "z too"))


def test_local_cutoff_roi_and_skip_value(ctx, before):
    """VR_GAMMA_LOCAL with zeros and negatives in R (T = tol * r is not > 0: skipped); a cutoff; an ROI contour holding NaN (in) and -0.0f
    (out); skipped voxels store a signalling NaN with a payload, bit for bit, and count as stored, not as evaluated."""
    ref, ev = doses(SHAPE, 21)
    rng = np.random.default_rng(22)
    r = ref[..., 3]
    r[rng.random(SHAPE) < 0.1] = f32(0.0)
    r[rng.random(SHAPE) < 0.1] = f32(-0.0)
    r[rng.random(SHAPE) < 0.1] *= f32(-1.0)
    _, res, _ = check(ctx, ref, ev, before, mode=LOCAL, tol=0.03, skip_bits=PAYLOAD, what="local")
    assert 0 < res[1] < res[0] and res[1] == int((r > 0).sum())
    _, res, _ = check(ctx, ref, ev, before, cutoff=18.5, skip_bits=PAYLOAD, what="cutoff")
    assert res[1] == int((r >= f32(18.5)).sum()) > 0
    m = ev[..., 0]  # the ROI: contour 0 of the evaluated slot
    m[...] = np.where(rng.random(SHAPE) < 0.5, f32(1.0), f32(0.0))
    m[rng.random(SHAPE) < 0.1] = f32(np.nan)
    m[rng.random(SHAPE) < 0.1] = f32(-0.0)
    _, res, _ = check(ctx, ref, ev, before, roi=(1, 0), skip_bits=PAYLOAD, sub=2, what="roi")
    assert res[1] == int(gr.member(m).sum()) and np.isnan(m).any() and (vt.bits(m) == 0x80000000).any()
    _, res, _ = check(ctx, ref, ev, before, mode=LOCAL, tol=0.03, cutoff=10.0, roi=(1, 0), skip_bits=0xFFFFFFFF, forms=FORMS[:2] + FORMS[4:], what="all three")
    assert 0 < res[1] < int(gr.member(m).sum())


def test_hostile_values(ctx, before):
    """NaN, +-inf, denormals, signed zeros and huge values in E and R: a NaN or infinite candidate is ignored or wins as the header says,
    a voxel whose every g2 is NaN stores 0x7FC00000, an infinite G2 stores +inf; both count as nonfinite."""
    ref, ev = rc.hostile(SHAPE, 31), rc.hostile(SHAPE, 33)
    _, res, _ = check(ctx, ref, ev, before, what="hostile")
    assert res[3] > 0
    check(ctx, ref, ev, before, sub=2, reach=1500, chans=(2, 1, 3), what="hostile, interpolated")
    check(ctx, ref, ev, before, mode=LOCAL, tol=0.03, reach=2000, forms=FORMS[:2] + FORMS[2:3], what="hostile, local")
    tiny = np.zeros(SHAPE + (4,), f32)
    tiny.view(u32)[..., 3] = np.random.default_rng(34).integers(1, 1 << 23, SHAPE)  # denormals: T = tol * r is a denormal, invT huge or inf
    check(ctx, tiny, ev, before, mode=LOCAL, tol=0.5, what="denormal tolerances")
    nans = np.full(SHAPE + (4,), np.nan, f32)
    _, res, _ = check(ctx, ref, nans, before, what="every g2 is NaN")
    assert res[3] == res[1] > 0 and res[2] == 0 and res[4] == 0


def test_equal_doses_and_a_shifted_ramp(ctx, before):
    """E equal to R: every stored value is +0.0f and passed == evaluated.  E equal to R shifted one voxel along x on a linear ramp of 0.5
    per voxel: away from the x faces gamma is the lesser of the dose term 0.5 / T and the distance term."""
    ref, _ = doses(SHAPE, 41)
    want, res, _ = check(ctx, ref, ref.copy(), before, reach=6000, what="equal")
    assert not vt.bits(want[..., 0]).any() and res[1] == res[2] == res[0] and res[3:] == (0, 0)
    ramp = np.zeros(SHAPE + (4,), f32)
    ramp[..., 3] = (0.5 * np.arange(37, dtype=f32))[None, None, :]
    shifted = ramp.copy()
    shifted[..., 3] = ramp[..., 3] + f32(0.5)  # E(x) = R(x + 1)
    want, res, _ = check(ctx, ramp, shifted, before, dta=3000, reach=3000, tol=0.25, what="ramp")
    g = want[..., 0]
    assert np.abs(g[:, :, 1:] - 1.0 / 3.0).max() < 1e-6 and (g[:, :, 0] == f32(2.0)).all()  # (1 mm over 3 mm; at x = 0 the dose term 0.5 / T)
    check(ctx, ramp, shifted, before, dta=3000, reach=2000, sub=4, tol=0.25, box=((0, 8, 5), (37, 12, 8)), what="ramp, sub 4")


def test_in_place_and_a_fresh_destination(ctx, pair):
    """In place on the reference's channel and on the evaluated channel; both doses in one slot; an empty destination slot is created
    with the reference's dimensions and zeros, by a whole box, a partial box and an empty box."""
    ref, ev = pair
    check(ctx, ref, ev, None, reach=6000, chans=(3, 3, 3), slots=(0, 1, 0), what="on the reference")
    check(ctx, ref, ev, None, reach=6000, sub=2, chans=(3, 3, 3), slots=(0, 1, 1), what="on the evaluated")
    both = ref.copy()
    both[..., 2] = ev[..., 3]
    check(ctx, both, both, None, reach=3000, chans=(3, 2, 2), slots=(1, 1, 1), box=((2, 3, 1), (35, 20, 12)), what="one slot")
    for box in (((0, 0, 0), rc.n_of(SHAPE)), ((3, 2, 1), (36, 13, 7)), ((5, 0, 0), (5, 21, 13))):
        for flavour in (0, 1):
            with capi.Context(W, H, 0) as c:
                c.set_kernel_flavour(flavour)
                c.volume_upload(0, ref)
                c.volume_upload(1, ev)
                p = dict(spacing=S, dta=3000, reach=3000, sub=1, mode=GLOBAL, tol=0.6, cutoff=-np.inf, skip_bits=QNAN, roi=(-1, 0), lo=box[0], hi=box[1])
                res = c.volume_gamma(describe(c, (0, 1, 2), (3, 3, 1), p))
                want, want_res, want_cnt = gr.gamma(ref, ev, None, 3, 3, 1, S, 3000, 3000, tol=0.6, lo=box[0], hi=box[1])
                got = c.volume_download(2, SHAPE)
                assert np.array_equal(vt.bits(got), vt.bits(want)) and res.as_tuple() == want_res and c.gamma_counters() == want_cnt
                assert not vt.bits(got[..., [0, 2, 3]]).any()


def test_an_empty_box(ctx, pair, before):
    want, res, cnt = check(ctx, *pair, before, box=((4, 5, 6), (20, 5, 9)), what="empty")
    assert res == (0, 0, 0, 0, 0) and cnt == (0, 0, 0) and np.array_equal(vt.bits(want), vt.bits(before))


def test_the_largest_table(ctx):
    """Radius 8 on every axis at sub 4: offsets up to +-32 sub-steps, a halo of 9 voxels and 111.7 KiB of LDS in the default form, on a
    20 x 20 x 20 volume with a box of 4 x 4 x 4 so that the plain form stays in seconds."""
    shape = (20, 20, 20)
    ref, ev = doses(shape, 51, shift=1.2, noise=2.0)
    _, res, cnt = check(ctx, ref, ev, rc.arbitrary_bits(shape, 52), spacing=(1000, 1000, 1000), dta=3000, reach=8000, sub=4, tol=0.3,
                        box=((8, 7, 9), (12, 11, 13)), what="radius 8, sub 4")
    assert cnt[0] == 64 and cnt[2] == len(gr.table((1000, 1000, 1000), 3000, 8000, 4)[2]) > 130000 and cnt[2] <= 65 ** 3


def test_the_launch_loops_go_round(ctx):
    """33 x 177 x 177 voxels: 2 x 23 x 45 = 2070 tiles for the 2048 workgroups the default form launches at the most, 1 033 857 voxels for
    the 524 288 lanes of the plain form.  K = 7: the reach is one voxel on every axis."""
    shape = (177, 177, 33)
    assert 2 * 23 * 45 > 2048 and shape[0] * shape[1] * shape[2] > 524288
    rng = np.random.default_rng(65)
    ref, ev = np.zeros(shape + (4,), f32), np.zeros(shape + (4,), f32)
    ref[..., 3] = rng.normal(20.0, 5.0, shape).astype(f32)
    ev[..., 3] = (ref[..., 3] + rng.normal(0.0, 1.0, shape)).astype(f32)
    _, res, cnt = check(ctx, ref, ev, np.zeros(shape + (4,), f32), spacing=(1000, 1000, 1000), dta=1000, reach=1000, tol=1.0, what="round again")
    assert cnt == (ref[..., 3].size, ref[..., 3].size, 7) and 0 < res[2] < res[1]


# ---- the cases of tests/gamma_cases.py (tests/test_gamma.py shows on the CPU that each has the property it is here for) -----------------

@pytest.mark.parametrize("shape", gc.EDGE_SHAPES, ids=lambda s: "x".join(str(v) for v in s[::-1]))
def test_tile_edges(ctx, shape):
    """One below, at and one above the tile's 32, 8 and 4 outputs, axes of one voxel, one voxel in all, and two tiles and a tail on
    every axis at once; a reach of two voxels at sub 1 and 2 and of two and a half at sub 2, where the halo's third voxel is read: the
    halo is longer than an axis in ten of the fourteen."""
    ref, ev = gc.edge_doses(shape)
    before = rc.arbitrary_bits(shape, 13)
    last = shape == gc.EDGE_SHAPES[-1]
    for sub, p in gc.EDGE_RUNS:
        check(ctx, ref, ev, before, sub=sub, tol=gc.EDGE_TOL, forms=FORMS[:2] + (FORMS[4:5] if last else []), what=(shape, sub, p["reach"]), **p)
    if last:
        for sub, p in gc.EDGE_RUNS:
            _, res, _ = check(ctx, ref, ev, before, sub=sub, mode=LOCAL, tol=0.03, box=gc.EDGE_BOX, chans=(3, 3, 1), what=(shape, sub, "box"), **p)
            assert res[0] == res[1] == 5 * 4 * 4


@pytest.mark.parametrize("n", gc.RODS, ids=lambda n: "x".join(str(v) for v in n))
def test_rods(ctx, n):
    """Axes of 65535 voxels: 2048 tiles along x, 8192 along y, 16384 along z (the tile loop goes round), a reach of two voxels."""
    ref, ev = gc.rod_doses(n)
    before = rc.arbitrary_bits(ref.shape[:3], 72)
    _, res, _ = check(ctx, ref, ev, before, sub=1, tol=gc.ROD_TOL, forms=FORMS[:2] + FORMS[4:5], what=n, **gc.EDGE)
    assert 0 < res[2] < res[1]
    _, res, _ = check(ctx, ref, ev, before, sub=2, tol=gc.ROD_TOL, box=gc.rod_far_box(n), chans=(3, 3, 2), what=(n, "far end"), **gc.EDGE)
    assert 0 < res[2] < res[1]


def lone_gamma64(ref, ev, at, p, tol):
    """gamma at voxel `at` (z, y, x) at sub 1, in float64 from the definition."""
    o, d2, _ = gr.table(sub=1, **p)
    z, y, x = at
    best = np.inf
    for (i, j, k), d in zip(o.tolist(), d2.tolist()):
        q = (z + k, y + j, x + i)
        if all(0 <= v < m for v, m in zip(q, ref.shape[:3])):
            best = min(best, d / float(p["dta"]) ** 2 + ((float(ev[q + (3,)]) - float(ref[at + (3,)])) / float(f32(tol))) ** 2)
    return float(np.sqrt(best))


def test_a_lone_asker(ctx):
    """One lane asks for all 293 entries, every other lane of the launch for entry 0 alone: the 63 beside it compute in step with it
    and their minima of +0 do not move.  The other way round the outlier stops at entry 1.  With the outlier in the last partial tile of
    a box off the tile origin the lanes beside it lie beyond the box."""
    cases = gc.lone_cases()
    zeros = np.zeros(gc.LONE_SHAPE + (4,), f32)
    for name in ("r", "e", "r_box"):
        ref, ev, at, box = cases[name]
        want, res, cnt = check(ctx, ref, ev, zeros, tol=gc.LONE_TOL, box=box, what=name, **gc.LONE)
        stored = vt.bits(want[..., 0])
        assert np.count_nonzero(stored) == 1 and not vt.bits(want[..., 1:]).any() and cnt[2] == 293 and res[1] == res[0], name
        if name == "e":
            assert stored[at] == vt.bits(np.sqrt(gr.table(sub=1, **gc.LONE)[2][1:2]))[0] and res[2] == res[1]
        else:
            g = lone_gamma64(ref, ev, at, gc.LONE, gc.LONE_TOL)
            assert abs(float(want[at + (0,)]) - g) <= 4e-7 * g and g > 100.0 and res[2] == res[1] - 1, (name, g)  # (a few roundings of 2^-24)
    ref, ev, at, _ = cases["r"]
    want, res, _ = check(ctx, ref, ev, zeros, tol=gc.LONE_TOL, sub=2, what="r, sub 2", **gc.LONE_SUB2)
    assert np.count_nonzero(vt.bits(want[..., 0])) == 1 and want[at + (0,)] > 100.0


@pytest.mark.parametrize("sub", [1, 2])
def test_exact_ties(ctx, sub):
    """Integer doses and integer c: in three voxels of four the running minimum equals the c of the entry that ends the search, bit
    for bit (`c < best` is strict, and the lanes that finished keep computing with minima that must not move)."""
    ref, ev = gc.tie_doses()
    _, res, cnt = check(ctx, ref, ev, rc.arbitrary_bits(gc.TIE_SHAPE, 14), sub=sub, tol=gc.TIE_TOL, what=("ties", sub), **gc.TIES[sub])
    assert cnt[2] == {1: 123, 2: 925}[sub] and 0 < res[2] < res[1] and res[3] == 0


def test_the_roi_may_be_the_destination(ctx, pair, before):
    """The ROI is the very contour the result overwrites (with NaN, in, and -0.0f, out); and the ROI lies in a third slot while the
    result overwrites R."""
    ref, ev = pair
    rng = np.random.default_rng(15)
    m = np.where(rng.random(SHAPE) < 0.5, f32(1.0), f32(0.0)).astype(f32)
    m[rng.random(SHAPE) < 0.1] = f32(np.nan)
    m[rng.random(SHAPE) < 0.1] = f32(-0.0)
    mine = before.copy()
    mine[..., 1] = m
    _, res, _ = check(ctx, ref, ev, mine, reach=6000, roi=(2, 1), chans=(3, 3, 1), skip_bits=PAYLOAD, what="roi is dst")
    assert res[1] == int(gr.member(m).sum()) and 0 < res[1] < res[0] and np.isnan(m).any() and (vt.bits(m) == 0x80000000).any()
    _, res, _ = check(ctx, ref, ev, mine, sub=2, roi=(2, 1), chans=(3, 3, 1), skip_bits=0, what="roi is dst, sub 2")
    third = rc.volume(SHAPE, 16)
    third[..., 2] = m
    _, res, _ = check(ctx, ref, ev, None, reach=6000, roi=(2, 2), chans=(3, 3, 3), slots=(0, 1, 0), skip_bits=PAYLOAD, extra={2: third}, what="third slot")
    assert res[1] == int(gr.member(m).sum())


def test_a_slot_of_four_gib():
    """A slot of 512 x 512 x 1032 voxels, 4.03 GiB: R in channel 3, E in channel 2, gamma into channel 0 of the same slot, in a box of
    five slabs across voxel index 2^28 (the start of slab z = 1024).  3 mm / 3 mm at 1 x 1 x 3 mm: 31 offsets, one slab along z, so the
    box equals the restatement of the slabs z0 - 1 .. z1 + 1 alone; every slab near the box and every 16th slab of the rest against the
    source."""
    shape = (ie.A1[2], ie.A1[1], ie.A1[0])
    z0, z1 = ie.LINE_Z - 2, ie.LINE_Z + 3
    lo, hi = (100, 200, z0), (391, 263, z1)
    band, ev = doses((z1 - z0 + 8, shape[1], shape[2]), 81)
    band[..., 2] = ev[..., 3]
    del ev
    src = np.zeros(shape + (4,), f32)
    src[z0 - 4:z1 + 4] = band
    sub = src[z0 - 1:z1 + 1]
    want, want_res, want_cnt = gr.gamma(sub, sub, sub, 3, 2, 0, S, 3000, 3000, tol=0.6, lo=(lo[0], lo[1], 1), hi=(hi[0], hi[1], 1 + z1 - z0))
    assert want_cnt == (291 * 63 * 5, 291 * 63 * 5, 31) and 0 < want_res[2] < want_res[1] and gr.radii(S, 3000)[2] == 1
    with capi.Context(W, H, 0) as c:
        c.volume_upload(0, src)
        for flavour in (0, 1):
            c.set_kernel_flavour(flavour)
            d = c.gamma_whole(0, 3, 0, 2, 0, 0).copy(spacing=S, dta=3000, reach=3000, dose_tolerance=0.6, box_lo=lo, box_hi=hi)
            res = c.volume_gamma(d)
            assert res.as_tuple() == want_res and c.gamma_counters() == want_cnt, flavour
            got = c.volume_download(0, shape)
            assert np.array_equal(vt.bits(got[z0:z1]), vt.bits(want[1:1 + z1 - z0])), flavour
            for sl in (slice(z0 - 8, z0), slice(z1, shape[0]), slice(0, z0 - 8, 16)):
                assert np.array_equal(vt.bits(got[sl]), vt.bits(src[sl])), (flavour, sl)
            del got
            if flavour == 0:
                c.volume_upload(0, src)


def test_everything_derived_is_fresh():
    """After a gamma into channel 3 of a rendered slot the next vr_render equals the oracle's frame for the restatement's volume, and the
    other tools' reports stay what they were."""
    n = 24
    shape = (n, n, n)
    v = ob.normalize_data(hr.raw_to_vec4(hr.ct_phantom_raw(n)))
    e = v.copy()
    e[..., 3] = f32(1.0) - v[..., 3]
    tf = (hr.default_opacity_tf(256), hr.default_color_tf(256))
    step, count = hr.stepping_params(n, n, n)
    u = hr.make_uniforms(W, H, steps_count=count, step_size=step)
    p = dict(spacing=(1000, 1000, 1000), dta=2000, reach=2000)
    want, want_res, want_cnt = gr.gamma(v, e, v, 3, 3, 3, tol=1.0, **p)
    assert 0.0 <= v[..., 3].min() and v[..., 3].max() <= 1.0 and want[..., 3].max() <= 1.0 and want_res[3] == 0  # (|1 - 2 v| <= 1 at the voxel itself)
    with capi.Context(W, H, 0) as c:
        c.volume_upload(0, v)
        c.volume_upload(1, e)
        c.tf_upload(0, *tf)
        c.set_uniforms(vt.to_capi_uniforms(u))
        c.render(capi.BASIC)
        before_frame = c.download()[0]
        tools = lambda: (c.morph_counters(), c.dist_counters(), c.resample_counters(), c.mesh_counters(), c.grow_counters(), c.hist_counters(),
                         c.filter_counters(), c.rank_counters())
        seen = tools()
        assert c.gamma_counters() == (0, 0, 0) and c.gamma_timing() == (0.0, 0.0, 0.0, 0.0)
        res = c.volume_gamma(c.gamma_whole(0, 3, 1, 3, 0, 3).copy(dose_tolerance=1.0, **p))
        assert res.as_tuple() == want_res and c.gamma_counters() == want_cnt
        assert seen == tools()
        c.render(capi.BASIC)
        frame, _, samples = c.download()
        assert np.array_equal(vt.bits(c.volume_download(0, shape)), vt.bits(want))
    ref, n_ref, _ = ob.render(ob.BASIC, u, [want], [tf], W, H, nthreads=4)
    assert samples == n_ref and n_ref > 0
    assert np.array_equal(vt.bits(frame), vt.bits(ref)) and not np.array_equal(vt.bits(frame), vt.bits(before_frame))


SWEEP = gc.sweep()


@pytest.mark.parametrize("i", range(len(SWEEP)))
def test_random_sweep(i):
    case = SWEEP[i]
    slots, chans, roi, vols = gc.sweep_volumes(case)
    extra = {roi[0]: vols[roi[0]]} if roi[0] >= 0 and roi[0] not in slots else None
    with capi.Context(W, H, 0) as c:
        check(c, vols[slots[0]], vols[slots[1]], vols.get(slots[2]), case["spacing"], case["dta"], case["reach"], case["sub"], case["mode"], case["tol"],
              case["cutoff"], case["skip_bits"], roi, (case["lo"], case["hi"]), chans, slots, [(case["flavour"], case["layout"])], case, extra)


def test_timing_and_the_other_tools_reports(ctx, pair):
    ref, ev = pair
    with capi.Context(W, H, 0) as c:
        assert c.gamma_counters() == (0, 0, 0) and c.gamma_timing() == (0.0, 0.0, 0.0, 0.0)
        c.volume_upload(0, ref)
        c.volume_upload(1, ev)
        c.volume_rank(c.rank_whole(0, 3, 2, 0))
        seen = (c.rank_counters(), c.filter_counters(), c.resample_counters(), c.hist_counters())
        c.volume_gamma(c.gamma_whole(0, 3, 1, 3, 2, 1).copy(spacing=S, dta=3000, reach=6000, dose_tolerance=0.6))
        timing = c.gamma_timing()
        assert all(t >= 0.0 for t in timing) and timing[0] > 0.0 and timing[1] == 0.0 and timing[3] > 0.0
        assert seen == (c.rank_counters(), c.filter_counters(), c.resample_counters(), c.hist_counters())


def test_errors_leave_every_slot_untouched(ctx, pair, before):
    ref, ev = pair
    nx, ny, nz = rc.n_of(SHAPE)
    ctx.volume_upload(0, ref)
    ctx.volume_upload(1, ev)
    ctx.volume_upload(2, before)
    whole = ctx.gamma_whole(0, 3, 1, 3, 2, 0)
    assert (list(whole.spacing), whole.dta, whole.reach, whole.sub, whole.mode, whole.dose_tolerance, whole.cutoff, whole.roi_slot) == ([1, 1, 1], 1, 1, 1, GLOBAL, 1.0, -np.inf, -1)
    assert bytes(whole)[capi.GammaDesc.skip_value.offset:][:4] == QNAN.to_bytes(4, "little")
    assert list(whole.box_lo) == [0, 0, 0] and list(whole.box_hi) == [nx, ny, nz]
    good = whole.copy(spacing=S, dta=3000, reach=3000, dose_tolerance=0.6)
    assert ctx.lib.vr_volume_gamma(ctx.h, C.byref(good), C.byref(capi.GammaResult())) == capi.VR_OK
    after = ctx.volume_download(2, SHAPE)
    counters = ctx.gamma_counters()
    assert counters == (nx * ny * nz, nx * ny * nz, 31)
    invalid = [dict(ref_slot=-1), dict(ref_slot=3), dict(eval_slot=-1), dict(eval_slot=3), dict(dst_slot=-1), dict(dst_slot=3), dict(ref_channel=-1),
               dict(ref_channel=4), dict(eval_channel=-1), dict(eval_channel=4), dict(dst_channel=-1), dict(dst_channel=4), dict(roi_slot=-2),
               dict(roi_slot=3), dict(roi_slot=1, roi_contour=4), dict(roi_slot=1, roi_contour=-1), dict(spacing=(0, 1000, 3000)),
               dict(spacing=(1000, (1 << 20) + 1, 3000)), dict(dta=0), dict(dta=(1 << 24) + 1), dict(reach=0), dict(reach=(1 << 24) + 1),
               dict(sub=0), dict(sub=5), dict(sub=-1), dict(reach=9000), dict(spacing=(1000, 1000, 333)), dict(mode=2), dict(mode=-1),
               dict(box_lo=(-1, 0, 0)), dict(box_hi=(nx + 1, ny, nz)), dict(box_hi=(nx, ny, nz + 1)), dict(box_lo=(5, 0, 0), box_hi=(4, ny, nz))]
    for over in invalid:
        d = good.copy(**over)
        assert ctx.lib.vr_volume_gamma(ctx.h, C.byref(d), C.byref(capi.GammaResult())) == capi.VR_ERR_INVALID_ARG, over
        assert (ctx.lib.vr_last_error(ctx.h) or b"").decode().startswith("vr_volume_gamma"), over
        if set(over) <= {"spacing", "dta", "reach", "sub"}:  # (the restatement's ranges are the product's)
            assert not gr.valid(**{**dict(spacing=S, dta=3000, reach=3000, sub=1), **over}), over
    assert ctx.lib.vr_volume_gamma(ctx.h, None, None) == capi.VR_ERR_INVALID_ARG
    assert ctx.lib.vr_volume_gamma(None, C.byref(good), None) == capi.VR_ERR_INVALID_ARG
    assert ctx.lib.vr_gamma_counters(ctx.h, None) == capi.VR_ERR_INVALID_ARG and ctx.lib.vr_gamma_timing(ctx.h, None) == capi.VR_ERR_INVALID_ARG
    for bad in ((3, 3, 1, 3, 2, 0), (-1, 3, 1, 3, 2, 0), (0, 4, 1, 3, 2, 0), (0, 3, 3, 3, 2, 0), (0, 3, 1, -1, 2, 0), (0, 3, 1, 3, 3, 0), (0, 3, 1, 3, 2, 4)):
        assert ctx.lib.vr_gamma_whole(ctx.h, *bad, C.byref(capi.GammaDesc())) == capi.VR_ERR_INVALID_ARG, bad
    assert ctx.lib.vr_gamma_whole(ctx.h, 0, 3, 1, 3, 2, 0, None) == capi.VR_ERR_INVALID_ARG
    assert ctx.gamma_counters() == counters
    for slot, v in ((0, ref), (1, ev), (2, after)):
        assert np.array_equal(vt.bits(ctx.volume_download(slot, SHAPE)), vt.bits(v)), slot
    assert ctx.lib.vr_volume_gamma(ctx.h, C.byref(good.copy(reach=2000)), None) == capi.VR_OK  # (a NULL result is fine)
    assert ctx.gamma_counters() == (nx * ny * nz, nx * ny * nz, 13)
    with capi.Context(W, H, 0) as other:  # slots of other dimensions; empty dose and ROI slots
        other.volume_upload(0, ref)
        other.volume_upload(1, np.zeros((4, 4, 4, 4), f32))
        assert other.lib.vr_volume_gamma(other.h, C.byref(good.copy(dst_slot=0)), None) == capi.VR_ERR_INVALID_ARG  # (the evaluated slot's)
        assert other.lib.vr_volume_gamma(other.h, C.byref(good.copy(eval_slot=0, dst_slot=1)), None) == capi.VR_ERR_INVALID_ARG  # (the destination's)
        assert other.lib.vr_volume_gamma(other.h, C.byref(good.copy(eval_slot=0, dst_slot=0, roi_slot=1)), None) == capi.VR_ERR_INVALID_ARG  # (the ROI's)
        assert other.lib.vr_volume_gamma(other.h, C.byref(good.copy(eval_slot=2, dst_slot=0)), None) == capi.VR_ERR_NOT_READY
        err = other.lib.vr_last_error(other.h)
        assert err.startswith(b"vr_volume_gamma") and b"empty" in err
        assert other.lib.vr_volume_gamma(other.h, C.byref(good.copy(eval_slot=0, dst_slot=0, roi_slot=2)), None) == capi.VR_ERR_NOT_READY
        assert other.lib.vr_volume_gamma(other.h, C.byref(good.copy(ref_slot=2, eval_slot=0, dst_slot=0)), None) == capi.VR_ERR_NOT_READY
        assert other.lib.vr_gamma_whole(other.h, 2, 3, 0, 3, 0, 0, C.byref(capi.GammaDesc())) == capi.VR_ERR_NOT_READY
        assert other.gamma_counters() == (0, 0, 0) and other.gamma_timing() == (0.0, 0.0, 0.0, 0.0)
        assert np.array_equal(vt.bits(other.volume_download(0, SHAPE)), vt.bits(ref))
        with pytest.raises(capi.VrError):  # (the failed calls created nothing)
            other.volume_download(2, SHAPE)


def test_application_gamma():
    """Application::Gamma at 1 x 1 x 3 mm equals the restatement with millimetres as whole micrometres: the default reach is twice the
    distance to agreement and VR_GAMMA_GLOBAL; the options pass through; bad millimetres are VR_ERR_INVALID_ARG."""
    from volumerendering_amd import host
    shape = (9, 20, 33)
    ref, ev = doses(shape, 95)
    vol = ref.copy()  # R in channel 3, E in channel 2, the ROI in contour 0 of one slot: slot 0 is the scene's
    vol[..., 2] = ev[..., 3]
    vol[..., 0] = np.where(np.random.default_rng(96).random(shape) < 0.7, f32(1.0), f32(0.0))
    spacing = (1.0, 1.0, 3.0)
    with host.Application(W, H, 0) as app:
        app.OnStart(capi.BASIC, [host.VolumeFile.from_vec4(vol)])
        c = app.context()
        c.volume_upload(1, vol)
        res = app.gamma(1, 3, 1, 2, 2, 0, 0.6, 3.0, spacing=spacing)
        want, want_res, want_cnt = gr.gamma(vol, vol, None, 3, 2, 0, S, 3000, 6000, tol=f32(0.6))
        got = c.volume_download(2, shape)
        assert np.array_equal(vt.bits(got), vt.bits(want)) and res.as_tuple() == want_res and c.gamma_counters() == want_cnt
        res = app.gamma(1, 3, 1, 2, 2, 1, 0.03, 2.0006, spacing=spacing, reach_mm=3.0, sub=2, mode=LOCAL, cutoff=15.0, roi_slot=1, roi_contour=0,
                        skip_bits=PAYLOAD)
        want, want_res, want_cnt = gr.gamma(vol, vol, got, 3, 2, 1, S, 2001, 3000, 2, LOCAL, f32(0.03), 15.0, PAYLOAD, vol, 0)
        assert np.array_equal(vt.bits(c.volume_download(2, shape)), vt.bits(want)) and res.as_tuple() == want_res and c.gamma_counters() == want_cnt
        assert 0 < want_res[1] < want_res[0]
        unit = app.gamma(1, 3, 1, 2, 2, 0, 0.6, 1.0)  # (no spacing: 1 mm, reach 2 mm)
        assert c.gamma_counters()[2] == len(gr.table((1000, 1000, 1000), 1000, 2000, 1)[2]) == 33 and unit.stored == ref[..., 3].size
        for bad in (dict(dta_mm=0.0), dict(dta_mm=-1.0), dict(dta_mm=float("nan")), dict(dta_mm=float("inf")), dict(dta_mm=3.0, spacing=(1.0, 0.0, 1.0)),
                    dict(dta_mm=3.0, spacing=(1.0, float("nan"), 1.0)), dict(dta_mm=3.0, reach_mm=-1.0), dict(dta_mm=5.0), dict(dta_mm=3.0, sub=5),
                    dict(dta_mm=3.0, spacing=(1.0, 1.0, 2000.0)), dict(dta_mm=20000.0)):
            with pytest.raises(capi.VrError) as e:
                app.gamma(1, 3, 1, 2, 2, 0, 0.6, **bad)
            assert e.value.code == capi.VR_ERR_INVALID_ARG, bad
            assert "Application::Gamma" in str(e.value) or "vr_volume_gamma" in str(e.value), (bad, str(e.value))
