"""GPU side of connected components (vr_mask_components, csrc/vr_comp.h): the table, the result, the downloaded slot (all four components,
bit for bit) and the counters EQUAL to the numpy restatement (comp_ref.py, pinned on the CPU by tests/test_components.py) -- the 40 cases
of the sweep, hand-made shapes that break labellers, a mid-size case whose scans chain over several tiles and whose runs contend for one
root, the composition with vr_histogram, vr_segment_grow and the renderer, and the protocol.  Everything is exact."""
import ctypes as C

import numpy as np
import pytest

import comp_cases as cc
import comp_ref as cr
import host_ref as hr
import morph_cases as mc
import test_histogram_gpu as thg
import vrtest as vt
from volumerendering_amd import capi

pytestmark = pytest.mark.gpu
f32 = np.float32
W, H = 64, 48


def desc(shape, box=None, **over):
    """A descriptor of contour 0 of slot 0 over the whole volume unless a box is given: FACES, everything selected, nothing written."""
    d = capi.ComponentsDesc()
    d.src_slot, d.src_contour, d.connectivity, d.min_voxels, d.max_voxels = 0, 0, capi.COMP_FACES, 1, cr.U64_MAX
    d.dst_slot, d.label_slot, d.combine = -1, -1, capi.MORPH_REPLACE
    lo, hi = box if box else cc.whole(shape)
    return d.copy(box_lo=lo, box_hi=hi, **over)


def reference(d, src, before):
    return cr.components(src, before, d.src_contour, d.background, d.connectivity, tuple(d.box_lo), tuple(d.box_hi), d.min_voxels,
                         d.max_voxels, d.reject_faces, d.keep_largest, d.dst_contour if d.dst_slot >= 0 else None, d.combine,
                         d.label_channel if d.label_slot >= 0 else None)


def check(ctx, d, src, before=None, what=None, want=None):
    """One Context.mask_components against the restatement: the table and the result element for element, the written slot bit for
    bit, the counters.  `src`: the source slot's voxels; `before`: the written slot's before the call (None: an empty slot, or none
    written); `want`: the restatement of this very call where a test has it already.  Returns (the restatement's dict, the downloaded
    written slot or None)."""
    shape = src.shape[:3]
    want = want or reference(d, src, before)
    got = ctx.mask_components(d)
    cnt = ctx.components_counters()
    assert got["result"].as_tuple() == want["result"], (what, got["result"].as_tuple(), want["result"])
    assert got["components"] == want["table"], (what, [(i, a, b) for i, (a, b) in enumerate(zip(got["components"], want["table"])) if a != b][:3])
    assert cnt == want["counters"], (what, cnt, want["counters"])
    assert cnt[0] == int(np.prod([h - l for l, h in zip(d.box_lo, d.box_hi)])) and want["result"][0] <= cnt[1] <= want["result"][2]
    written = d.dst_slot if d.dst_slot >= 0 else d.label_slot
    after = None
    if written >= 0:
        after = ctx.volume_download(written, shape)
        bad = np.argwhere(vt.bits(after) != vt.bits(want["out"]))
        assert bad.size == 0, (what, len(bad), bad[:4])
    return want, after


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(W, H, 0)
    yield c
    c.close()


SWEEP = cc.sweep(40)


@pytest.mark.parametrize("i", range(40))
def test_random_sweep(i):
    case = SWEEP[i]
    src, before = cc.case_volumes(case)
    with capi.Context(W, H, 0) as c:
        c.volume_upload(case["src_slot"], src)
        if before is not None and case["dst_slot"] != case["src_slot"]:
            c.volume_upload(case["dst_slot"], before)
        slot = -1 if case["dst_slot"] is None else case["dst_slot"]
        d = capi.ComponentsDesc().copy(
            src_slot=case["src_slot"], src_contour=case["src_contour"], background=case["background"], connectivity=case["connectivity"],
            box_lo=case["box_lo"], box_hi=case["box_hi"], min_voxels=case["min_voxels"], max_voxels=case["max_voxels"],
            reject_faces=case["reject_faces"], keep_largest=case["keep_largest"], combine=case["combine"],
            dst_slot=slot if case["dst_contour"] is not None else -1, dst_contour=case["dst_contour"] or 0,
            label_slot=slot if case["label_channel"] is not None else -1, label_channel=case["label_channel"] or 0)
        check(c, d, src, before, what=case)
        if slot != case["src_slot"]:  # the source slot keeps its bits
            assert np.array_equal(vt.bits(c.volume_download(case["src_slot"], case["shape"])), vt.bits(src))


SHAPES = {"serpentine": cc.serpentine(), "comb_row": cc.comb(axis="row"), "comb_slice": cc.comb(axis="slice"),
          "checkerboard": cc.checkerboard(), "shells": cc.shells(), "corner_pair": cc.corner_pair()}


@pytest.mark.parametrize("name", list(SHAPES))
def test_shapes_that_break_labellers(ctx, name):
    a = SHAPES[name]
    shape = a.shape
    src = cc.volume(a, 0, seed=7)
    ctx.volume_upload(0, src)
    state = mc.arbitrary_bits(shape, seed=8)
    ctx.volume_upload(1, state)
    counts = {}
    for connectivity in cc.CONNECTIVITIES:
        for background in (0, 1):
            d = desc(shape, connectivity=connectivity, background=background, label_slot=1, label_channel=2, dst_slot=1, dst_contour=0,
                     keep_largest=1)
            want, state = check(ctx, d, src, state, what=(name, connectivity, background))
            counts[connectivity, background] = want["result"][0]
    n = int(a.sum())
    if name == "serpentine":
        assert counts[6, 0] == 1 and counts[4, 0] == 5
    if name == "comb_row":
        assert counts[6, 0] == 2 and counts[4, 0] == 2
    if name == "comb_slice":
        assert counts[6, 0] == 1 and counts[4, 0] > 30
    if name == "checkerboard":
        assert counts[6, 0] == n and counts[26, 0] == 1 and counts[6, 1] == a.size - n
    if name == "shells":
        assert counts[26, 0] == 3 and counts[6, 1] == 4
        # holes within holes: the components of the complement that touch no face, ORed in, give the solid cube
        d = desc(shape, background=1, reject_faces=63, dst_slot=0, dst_contour=0, combine=capi.MORPH_OR)
        want, after = check(ctx, d, src, src)
        assert want["result"][1] == 3 and int(cr.member(after[..., 0]).sum()) == 11 ** 3
    if name == "corner_pair":
        assert counts[6, 0] == 2 and counts[26, 0] == 1 and counts[8, 0] == 2


def test_chained_scan_and_contention(ctx):
    """(257, 33, 17) at density 0.32: the box has 5 words a row and 2805 words, three scan tiles; some 30000 runs, most of them in one
    component under 26 (0.32 is far above that lattice's percolation threshold, and just above the cubic lattice's 0.3116).  Twice: the
    outcome does not depend on how the unions interleave."""
    shape = (17, 33, 257)
    src = cc.volume(cc.random_set(shape, 0.32, 77), 1, seed=78)
    ctx.volume_upload(0, src)
    state = mc.arbitrary_bits(shape, seed=79)
    ctx.volume_upload(2, state)
    for connectivity in (capi.COMP_FACES, capi.COMP_ALL):
        d = desc(shape, src_contour=1, connectivity=connectivity, label_slot=2, label_channel=3, dst_slot=2, dst_contour=1, keep_largest=2,
                 combine=capi.MORPH_OR)
        first, state = check(ctx, d, src, state, what=connectivity)
        again, state = check(ctx, d, src, state, what=connectivity)
        assert first["result"] == again["result"] and first["counters"][1] > 2 * 1024  # (nodes: more than two scan tiles)
        if connectivity == capi.COMP_ALL:
            assert first["result"][4] > first["result"][2] // 2  # (one component holds most of S)


def test_composition_with_histogram_and_grow(ctx):
    shape = (9, 14, 67)
    a = cc.random_set(shape, 0.3, 91)
    src = cc.volume(a, 0, seed=92)
    ctx.volume_upload(0, src)
    ctx.volume_upload(1, np.zeros(shape + (4,), f32))
    for connectivity in (capi.COMP_FACES, capi.COMP_ALL):
        d = desc(shape, connectivity=connectivity, label_slot=1, label_channel=2, dst_slot=1, dst_contour=0, keep_largest=1)
        want, after = check(ctx, d, src, ctx.volume_download(1, shape))
        n = want["result"][0]
        # the histogram of the label channel: bin k holds component k's size, bin 0 the voxels outside S
        counts, rows = ctx.histogram(thg.desc(shape, volume_slot=1, channel=2, bins=n + 1, scale=1.0))
        assert counts[0].tolist() == [a.size - int(a.sum())] + [t[0] for t in want["table"]] and rows[0] == (a.size, 0)
        # the region grown from `first` of the largest component is what keep_largest = 1 kept
        big = max(range(n), key=lambda i: (want["table"][i][0], -i))
        binary = np.zeros(shape + (4,), f32)
        binary[..., 3] = a
        ctx.volume_upload(2, binary)
        res = ctx.segment_grow(ctx.grow_whole(2, 1, 3, 0.5, 1.5).copy(seeds=[want["table"][big][3]], connectivity=connectivity))
        both = ctx.volume_download(1, shape)
        grown = cr.member(both[..., 3])
        assert res.voxels == want["result"][4] and np.array_equal(grown, cr.member(both[..., 0])) and np.array_equal(grown, want["r"])


@pytest.mark.parametrize("variant", [capi.VOLUME_MASK, capi.TF_CALIB], ids=["volume_mask", "tf_calib"])
@pytest.mark.parametrize("layout", [0, 3])
def test_a_frame_after_the_call_is_the_frame_after_an_upload(variant, layout):
    """What is derived from the written slot is rebuilt: a frame after vr_mask_components equals the frame after vr_volume_upload of the
    same mask, bit for bit; what the reporting calls say about earlier launches and tools stays."""
    n = 16
    vols, tfs = vt.scene(variant, n)
    mslot = 0 if variant == capi.VOLUME_MASK else 1
    shape = vols[mslot].shape[:3]
    step, count = hr.stepping_params(n, n, n)
    u = hr.make_uniforms(W, H, steps_count=count, step_size=step)
    with capi.Context(W, H, 0) as c:
        c.set_volume_layout(layout)
        before_frame, _, _ = vt.gpu_render(c, variant, u, vols, tfs)
        # the counting call: no slot is written, nothing derived is touched
        d = desc(shape, src_slot=mslot, dst_slot=mslot, dst_contour=0, max_voxels=0)  # contour 0 cleared: nothing is that small
        out = capi.ComponentsResult()
        c._chk(c.lib.vr_mask_components(c.h, C.byref(d.copy(dst_slot=-1)), C.byref(out)))
        assert out.n_components >= 1 and c.components_timing()[3] == 0.0
        assert np.array_equal(vt.bits(c.volume_download(mslot, shape)), vt.bits(vols[mslot]))
        c.render(variant)
        assert np.array_equal(vt.bits(c.download()[0]), vt.bits(before_frame))
        reports = (c.counters(), c.last_kernel_flavour(), len(c.kernel_times()), c.morph_counters(), c.outlines_counters())
        want, mask = check(c, d, vols[mslot], vols[mslot])
        assert want["result"][1] == 0 and not cr.member(mask[..., 0]).any() and cr.member(vols[mslot][..., 0]).any()
        timing = c.components_timing()
        assert len(timing) == 4 and all(t >= 0.0 for t in timing) and timing[3] > 0.0
        assert (c.counters(), c.last_kernel_flavour(), len(c.kernel_times()), c.morph_counters(), c.outlines_counters()) == reports
        c.render(variant)
        frame = c.download()[0]
        c.volume_upload(mslot, mask)
        c.render(variant)
        uploaded = c.download()[0]
    assert np.array_equal(vt.bits(frame), vt.bits(uploaded))
    assert not np.array_equal(vt.bits(frame), vt.bits(before_frame))  # (the cleared contour shows)


def test_protocol_and_errors(ctx):
    shape = (5, 9, 70)
    nz, ny, nx = shape
    a = cc.random_set(shape, 0.3, 51)
    src = cc.volume(a, 0, seed=52)
    m = mc.arbitrary_bits(shape, seed=53)
    with capi.Context(W, H, 0) as empty:
        assert empty.components_counters() == (0, 0, 0) and empty.components_timing() == (0.0, 0.0, 0.0, 0.0)
        assert empty.lib.vr_mask_components(empty.h, C.byref(desc(shape)), None) == capi.VR_ERR_NOT_READY
        err = empty.lib.vr_last_error(empty.h)
        assert err.startswith(b"vr_mask_components") and b"empty" in err
        assert empty.lib.vr_components_whole(empty.h, 0, 0, C.byref(capi.ComponentsDesc())) == capi.VR_ERR_NOT_READY
    ctx.volume_upload(0, src)
    ctx.volume_upload(1, m)
    ctx.volume_upload(2, np.zeros((4, 4, 4, 4), f32))
    good = desc(shape, dst_slot=1, dst_contour=1, label_slot=1, label_channel=3)
    want, m = check(ctx, good, src, m)
    n = want["result"][0]
    counters = ctx.components_counters()
    assert n > 10 and ctx.components_timing()[3] > 0.0

    def untouched():
        assert np.array_equal(vt.bits(ctx.volume_download(1, shape)), vt.bits(m))
        assert np.array_equal(vt.bits(ctx.volume_download(0, shape)), vt.bits(src))
        assert np.array_equal(vt.bits(ctx.volume_download(2, (4, 4, 4))), np.zeros((4, 4, 4, 4), np.uint32))

    # the counting call writes no slot; ms[3] == 0 for a call that writes nothing
    out = capi.ComponentsResult()
    assert ctx.lib.vr_mask_components(ctx.h, C.byref(desc(shape, connectivity=26)), C.byref(out)) == capi.VR_OK
    assert out.as_tuple() == reference(desc(shape, connectivity=26), src, None)["result"] and ctx.components_timing()[3] == 0.0
    untouched()
    # a table that is too small: the table and the slots untouched, the result filled, the count named
    table = (capi.Component * n)()
    C.memset(table, 0xAB, C.sizeof(table))
    image = bytes(table)
    out = capi.ComponentsResult()
    small = good.copy(max_components=n - 1, components=C.cast(table, C.c_void_p).value, keep_largest=3, combine=capi.MORPH_ANDNOT)
    assert ctx.lib.vr_mask_components(ctx.h, C.byref(small), C.byref(out)) == capi.VR_ERR_INVALID_ARG
    err = ctx.lib.vr_last_error(ctx.h).decode()
    assert err.startswith("vr_mask_components") and f" {n} components" in err and str(n - 1) in err
    assert bytes(table) == image and out.as_tuple() == reference(small, src, m)["result"] and out.n_selected == 3
    untouched()
    # ... and one that is large enough is filled up to n
    big = (capi.Component * (n + 2))()
    C.memset(big, 0xAB, C.sizeof(big))
    assert ctx.lib.vr_mask_components(ctx.h, C.byref(desc(shape, max_components=n + 2, components=C.cast(big, C.c_void_p).value)), None) == capi.VR_OK
    assert [q.as_tuple() for q in big[:n]] == want["table"] and bytes(big)[n * 48:] == b"\xab" * 96
    counters = ctx.components_counters()

    invalid = [dict(src_slot=-1), dict(src_slot=3), dict(dst_slot=-2), dict(dst_slot=3), dict(label_slot=-2), dict(label_slot=3),
               dict(src_contour=-1), dict(src_contour=4), dict(dst_contour=-1), dict(dst_contour=4), dict(label_channel=-1),
               dict(label_channel=4), dict(background=2), dict(background=-1), dict(connectivity=0), dict(connectivity=18),
               dict(connectivity=5), dict(combine=-1), dict(combine=4), dict(keep_largest=65), dict(reject_faces=64),
               dict(reject_faces=1 << 31), dict(box_lo=(-1, 0, 0)), dict(box_hi=(nx + 1, ny, nz)), dict(box_hi=(nx, ny, nz + 1)),
               dict(box_lo=(5, 0, 0), box_hi=(4, ny, nz)),
               dict(label_slot=0),                      # the contour and the label map in different slots
               dict(label_channel=1),                   # ... in the same component
               dict(dst_slot=2, label_slot=2),          # a destination of other dimensions
               dict(dst_slot=-1, label_slot=2), dict(dst_slot=2, label_slot=-1),
               dict(max_components=5),                  # a capacity without a pointer
               dict(components=C.cast(table, C.c_void_p).value)]  # a pointer without a capacity
    for over in invalid:
        d = good.copy(**over)
        assert ctx.lib.vr_mask_components(ctx.h, C.byref(d), C.byref(capi.ComponentsResult())) == capi.VR_ERR_INVALID_ARG, over
        assert (ctx.lib.vr_last_error(ctx.h) or b"").decode().startswith("vr_mask_components"), over
    assert ctx.lib.vr_mask_components(ctx.h, None, None) == capi.VR_ERR_INVALID_ARG
    assert ctx.lib.vr_mask_components(None, C.byref(good), None) == capi.VR_ERR_INVALID_ARG
    assert ctx.lib.vr_components_counters(ctx.h, None) == capi.VR_ERR_INVALID_ARG
    assert ctx.lib.vr_components_timing(ctx.h, None) == capi.VR_ERR_INVALID_ARG
    assert ctx.components_counters() == counters and bytes(table) == image
    untouched()
    # vr_components_whole
    assert bytes(ctx.components_whole(0, 2)) == bytes(desc(shape, src_contour=2))
    for bad in ((3, 0), (-1, 0), (0, 4), (0, -1)):
        assert ctx.lib.vr_components_whole(ctx.h, *bad, C.byref(capi.ComponentsDesc())) == capi.VR_ERR_INVALID_ARG, bad
    assert ctx.lib.vr_components_whole(ctx.h, 0, 0, None) == capi.VR_ERR_INVALID_ARG
    # an empty box and an empty contour: zero components and VR_OK; what was asked for is still written over the box
    for box in (((3, 2, 1), (3, ny, nz)), ((0, 0, 2), (nx, ny, 2))):
        want, _ = check(ctx, good.copy(box_lo=box[0], box_hi=box[1]), src, m)
        assert want["result"] == (0, 0, 0, 0, 0, (0, 0, 0), (0, 0, 0)) and want["counters"] == (0, 0, 0)
    ctx.volume_upload(0, np.zeros(shape + (4,), f32))
    want, m2 = check(ctx, good, np.zeros(shape + (4,), f32), m)
    assert want["result"][0] == 0 and not m2[..., 1].any() and not m2[..., 3].any()
    want, _ = check(ctx, good.copy(background=1, connectivity=4), np.zeros(shape + (4,), f32), m2)
    assert want["result"][0] == nz and want["table"][0][4] == 0b011111  # a full slice touches every face but the far z one


def test_timing_and_counters_of_every_ending(ctx):
    """What vr_components_timing and vr_components_counters report after each ending a small input reaches, on (5, 12, 30) voxels: a
    call that writes no slot times three phases and leaves the fourth at exactly 0.0, with VR_OK or with a table too small; one that
    writes a slot times all four, and with a table too small none; the counters are the call's own; an argument error leaves both as
    they were."""
    shape = (5, 12, 30)
    nz, ny, nx = shape
    src = cc.volume(cc.random_set(shape, 0.3, 61), 0, seed=62)
    m = mc.arbitrary_bits(shape, seed=63)
    ctx.volume_upload(0, src)
    ctx.volume_upload(1, m)
    ctx.volume_upload(2, np.zeros(shape + (4,), f32))
    d = desc(shape)
    part = desc(shape, ((2, 1, 1), (nx, ny - 2, 3)))
    empty = desc(shape, ((3, 2, 1), (3, ny, nz)))
    (n, cnt_d), (n2, cnt_part) = ((w["result"][0], w["counters"]) for w in (reference(x, src, None) for x in (d, part)))
    assert n > 10 and 1 < n2 < n and cnt_part[0] < cnt_d[0]
    table = (capi.Component * n)()

    def ended(x, capacity, rc, began, counted, what):
        got = ctx.lib.vr_mask_components(ctx.h, C.byref(x.copy(max_components=capacity, components=C.cast(table, C.c_void_p).value if capacity else None)),
                                         C.byref(capi.ComponentsResult()))
        ms, cnt = ctx.components_timing(), ctx.components_counters()
        assert got == rc, (what, got)
        assert all(t >= 0.0 for t in ms[:began]) and ms[began:] == (0.0,) * (4 - began), (what, ms)
        assert began < 4 or ms[3] > 0.0, (what, ms)
        assert cnt == counted, (what, cnt)

    def argument_error(what):
        before = ctx.components_timing(), ctx.components_counters()
        assert ctx.lib.vr_mask_components(ctx.h, C.byref(d.copy(connectivity=5)), None) == capi.VR_ERR_INVALID_ARG
        assert (ctx.components_timing(), ctx.components_counters()) == before, what

    into = dict(dst_slot=1, dst_contour=1, label_slot=1, label_channel=3)
    ended(d.copy(**into), n, capi.VR_OK, 4, cnt_d, "a slot written, exact capacity")
    argument_error("after a call that wrote a slot")
    ended(part, 0, capi.VR_OK, 3, cnt_part, "no slot, the counting call")
    ended(d, n, capi.VR_OK, 3, cnt_d, "no slot, exact capacity")
    ended(part, n2 - 1, capi.VR_ERR_INVALID_ARG, 3, cnt_part, "no slot, the table one short")
    argument_error("after a table too small")
    ended(empty, 0, capi.VR_OK, 3, (0, 0, 0), "no slot, empty box")
    ended(d.copy(src_slot=2), 0, capi.VR_OK, 3, (cnt_d[0], 0, 0), "no slot, contour empty in the box")
    ended(part.copy(**into), n2 - 1, capi.VR_ERR_INVALID_ARG, 0, cnt_part, "a slot written, the table one short")
    argument_error("after a refused write")
    ended(empty.copy(**into), 0, capi.VR_OK, 4, (0, 0, 0), "a slot written, empty box")
