"""Connected components (vr_mask_components, csrc/vr_comp.h) at the sizes where its kernels take another path, still EQUAL to the numpy
restatement: 65535-voxel axes (a node's first and last x in 16 bits each, runs over 1024 words, 65535 rows or slices); masks with more
than comp_cases.LANE_CAP nodes and components, so that every grid-stride loop goes round again; scans of exactly one spine chunk and of
one word more; and the label limit, 2^24 components with a label map, from both sides.  The thresholds are comp_cases' and are checked
against the headers by tests/test_components.py, which also asserts what each case here must contain."""
import ctypes as C

import numpy as np
import pytest

import comp_cases as cc
import comp_ref as cr
import morph_cases as mc
import vrtest as vt
from test_components_gpu import check, desc
from volumerendering_amd import capi

pytestmark = pytest.mark.gpu
f32 = np.float32
W, H = 64, 48
COMPONENT = np.dtype([("voxels", "<u8"), ("lo", "<i4", (3,)), ("hi", "<i4", (3,)), ("first", "<i4", (3,)), ("faces", "<u4")])  # vr_component


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(W, H, 0)
    yield c
    c.close()


def call(ctx, d, capacity=0):
    """One vr_mask_components through the library with a table of `capacity` entries (0: none): (the return code, the result as a
    tuple, the table as a structured array or None, the counters)."""
    table = (capi.Component * capacity)() if capacity else None
    out = capi.ComponentsResult()
    d = d.copy(max_components=capacity, components=C.cast(table, C.c_void_p).value if capacity else None)
    rc = ctx.lib.vr_mask_components(ctx.h, C.byref(d), C.byref(out))
    return rc, out.as_tuple(), (np.frombuffer(table, COMPONENT) if capacity else None), ctx.components_counters()


def check_arrays(ctx, d, want, shape, what):
    """One call against comp_cases.reference_arrays' dict: the table column by column, the result, the counters and the written slot
    bit for bit.  Returns the table's bytes."""
    n = want["result"][0]
    rc, result, table, counters = call(ctx, d, n)
    assert rc == capi.VR_OK, (what, rc, ctx.lib.vr_last_error(ctx.h))
    assert result == want["result"], (what, result, want["result"])
    assert counters == want["counters"], (what, counters, want["counters"])
    assert COMPONENT.itemsize == C.sizeof(capi.Component) == 48 and len(table) == n
    for name, col in zip(("voxels", "lo", "hi", "first", "faces"), want["table"]):
        bad = np.flatnonzero((table[name].astype(np.int64) != col).reshape(n, -1).any(axis=1))
        assert bad.size == 0, (what, name, len(bad), bad[:4], table[name][bad[:4]], col[bad[:4]])
    written = d.dst_slot if d.dst_slot >= 0 else d.label_slot
    after = ctx.volume_download(written, shape)
    bad = np.argwhere(vt.bits(after) != vt.bits(want["out"]))
    assert bad.size == 0, (what, len(bad), bad[:4])
    return table.tobytes()


@pytest.mark.parametrize("background", [0, 1])
@pytest.mark.parametrize("connectivity", cc.CONNECTIVITIES)
@pytest.mark.parametrize("name", list(cc.RODS))
def test_rods_of_65535(ctx, name, connectivity, background):
    """One axis of 65535 voxels (comp_cases.rod): the set or its complement, over the whole box and over the box that cuts one voxel
    off each end of the long axis (for an x rod a partial first word and hi[0] = 65534), a contour of the three largest and a label map
    written into a slot of arbitrary bits; the cut box also rejects, in one call, the two faces of the long axis."""
    shape = cc.RODS[name]
    src = cc.volume(cc.rod(name), 0, seed=31)
    ctx.volume_upload(0, src)
    state = mc.arbitrary_bits(shape, seed=32)
    ctx.volume_upload(1, state)
    axis = cc.rod_axis(name)
    whole_box, cut_box = cc.rod_boxes(name)
    for box, reject in ((whole_box, 0), (cut_box, 3 << (2 * axis))):
        d = desc(shape, box=box, connectivity=connectivity, background=background, keep_largest=3, reject_faces=reject, dst_slot=1,
                 dst_contour=3, label_slot=1, label_channel=1)
        want, state = check(ctx, d, src, state, what=(name, connectivity, background, box))
        if not background and box == whole_box and connectivity == cr.FACES:
            assert want["result"][0] >= 1000 and want["result"][4] >= cc.AXIS  # (many components; one spans the long axis)
        if not background and name == "z" and connectivity == cr.PLANE_FACES:
            assert want["result"][0] >= cc.AXIS - 2 * (box == cut_box)  # (no path crosses slices)


@pytest.mark.parametrize("name", list(cc.MIDDLE))
def test_more_nodes_than_lanes(ctx, name):
    """The middle-scale masks (comp_cases.MIDDLE; their counts are pinned by tests/test_components.py): more than LANE_CAP nodes, and
    for the FACES checkerboard as many components, so every comp_* kernel's loop goes round at least twice and both scans chain over
    more than one spine chunk.  Twice: the table does not depend on how the unions and the statistics' atomics interleave."""
    make, connectivity, keep = cc.MIDDLE[name]
    a = make()
    shape = a.shape
    src = cc.volume(a, 2, seed=41)
    state = mc.arbitrary_bits(shape, seed=42)
    ctx.volume_upload(0, src)
    ctx.volume_upload(1, state)
    d = desc(shape, src_contour=2, connectivity=connectivity, keep_largest=keep, dst_slot=1, dst_contour=0, label_slot=1, label_channel=3)
    want = cc.reference_arrays(src, state, 2, 0, connectivity, tuple(d.box_lo), tuple(d.box_hi), keep_largest=keep, dst_contour=0,
                               label_channel=3)
    assert want["counters"][1] > cc.LANE_CAP
    first = check_arrays(ctx, d, want, shape, what=name)
    print("vr_components_timing", name, want["result"][0], "components", want["counters"][1], "nodes:",
          " ".join("%.3f" % t for t in ctx.components_timing()), "ms")
    again = check_arrays(ctx, d, want, shape, what=(name, "again"))  # (REPLACE over the box and the labels: the same slot after as before)
    assert first == again
    if name == "checkerboard_faces":  # ties go to the smaller label: the winners are the first 64 set voxels in raster order
        assert want["selected"].tolist() == list(range(64)) and want["result"][1] == 64
        assert np.array_equal(np.flatnonzero(want["r"]), np.flatnonzero(a)[:64])
    assert np.array_equal(vt.bits(ctx.volume_download(0, shape)), vt.bits(src))


@pytest.mark.parametrize("name", list(cc.SCAN_BOXES))
def test_scan_of_one_spine_chunk_and_one_word_more(ctx, name):
    """(8, 545, 512) voxels, one word a row: a box of exactly 262 144 words -- 256 scan tiles, one full round of scan_spine_kernel's
    loop -- and one of 262 145; the scan over the nodes (some 465 000) takes two rounds in both.  FACES: the restatement needs about
    four seconds for either box."""
    shape = cc.SCAN_SHAPE
    box = cc.SCAN_BOXES[name]
    src = cc.volume(cc.random_set(shape, cc.SCAN_DENSITY, cc.SCAN_SEED), 1, seed=51)
    state = mc.arbitrary_bits(shape, seed=52)
    ctx.volume_upload(0, src)
    ctx.volume_upload(2, state)
    d = desc(shape, box=box, src_contour=1, keep_largest=7, dst_slot=2, dst_contour=2, label_slot=2, label_channel=0)
    want = cc.reference_arrays(src, state, 1, 0, cr.FACES, *box, keep_largest=7, dst_contour=2, label_channel=0)
    assert cc.box_words(shape, *box) == cc.SCAN_TILE * cc.SPINE_CHUNK + (name == "one_more")
    assert want["counters"][1] > cc.SCAN_TILE * cc.SPINE_CHUNK and want["result"][0] > 100 * cc.SCAN_TILE
    check_arrays(ctx, d, want, shape, what=name)


# ---- the label limit -----------------------------------------------------------------------------------------------------------------

def slabs_differ(got, want, step=10):
    """The first (z, y, x, c) at which two volumes' bits differ, or None; ten slices at a time."""
    for z in range(0, got.shape[0], step):
        bad = np.argwhere(vt.bits(got[z:z + step]) != vt.bits(want[z:z + step]))
        if bad.size:
            return (int(bad[0][0]) + z,) + tuple(int(q) for q in bad[0][1:]), len(bad)
    return None


def test_label_limit_from_both_sides():
    """The FACES checkerboard of (512, 512, 130) in contour 0 of a 520 MiB slot whose other components are +0.0f: 131 072 isolated
    voxels a slice, so 128 slices hold exactly VR_COMP_MAX_LABEL = 2^24 components and 129 hold 131 072 more.  The reference is the
    closed form comp_cases.isolated_labels (pinned to the restatement by tests/test_components.py).  Three calls: the label map at the
    limit; one slice beyond it, refused with the result filled and nothing written; and a contour beyond it, which no f32 stores."""
    nz, ny, nx = shape = cc.LIMIT_SHAPE
    per_slice = ny * nx // 2
    assert 128 * per_slice == capi.COMP_MAX_LABEL
    v = np.zeros(shape + (4,), f32)
    v[..., 0] = (np.arange(nz)[:, None, None] + np.arange(ny)[None, :, None] + np.arange(nx)[None, None, :]) % 2 == 0
    with capi.Context(W, H, 0) as c, capi.Context(W, H, 0) as other:
        c.volume_upload(0, v)
        other.volume_upload(0, v)
        # 1. exactly 2^24 components: labels up to 16777216.0f
        d = desc(shape, box=((0, 0, 0), (nx, ny, 128)), label_slot=0, label_channel=2)
        rc, result, _, counters = call(c, d)
        assert rc == capi.VR_OK, c.lib.vr_last_error(c.h)
        n = 1 << 24
        assert result == (n, n, n, n, 1, (0, 0, 0), (nx, ny, 128)) and counters == (2 * n, n, 0)
        print("vr_components_timing label map of 2^24 components:", " ".join("%.3f" % t for t in c.components_timing()), "ms")
        for z in range(128):  # v becomes what the slot must hold now
            v[z, :, :, 2] = (cc.isolated_labels(v[z, :, :, 0] != 0) + z * per_slice) * (v[z, :, :, 0] != 0)
        last = np.flatnonzero(v[127, :, :, 0])[-2:]
        assert v[127, :, :, 2].ravel()[last].tolist() == [16777215.0, 16777216.0] and v[127, :, :, 2].max() == 16777216.0
        assert v[0, 0, 0, 2] == 1.0 and v[0, 0, 2, 2] == 2.0 and not v[128:, :, :, 2].any()
        assert slabs_differ(c.volume_download(0, shape), v) is None
        # 2. one slice more: refused, the result filled, nothing written, an empty label slot still empty
        more = n + per_slice
        d = desc(shape, box=((0, 0, 0), (nx, ny, 129)), label_slot=0, label_channel=2)
        for ctx, dd in ((c, d), (other, d.copy(label_slot=1))):
            rc, result, _, counters = call(ctx, dd)
            assert rc == capi.VR_ERR_UNSUPPORTED
            err = ctx.lib.vr_last_error(ctx.h).decode()
            assert err.startswith("vr_mask_components") and f" {more} components" in err, err
            assert result == (more, more, more, more, 1, (0, 0, 0), (nx, ny, 129)) and counters == (2 * more, more, 0)
        assert slabs_differ(c.volume_download(0, shape), v) is None
        assert other.lib.vr_components_whole(other.h, 1, 0, C.byref(capi.ComponentsDesc())) == capi.VR_ERR_NOT_READY  # (still empty)
        # 3. beyond the limit without a label map: a contour of the 64 largest, which ties give to the first 64 set voxels
        d = desc(shape, box=((0, 0, 0), (nx, ny, 129)), keep_largest=64, dst_slot=0, dst_contour=1)
        rc, result, _, counters = call(c, d)
        assert rc == capi.VR_OK, c.lib.vr_last_error(c.h)
        assert result == (more, 64, more, 64, 1, (0, 0, 0), (127, 1, 1)) and counters == (2 * more, more, 0)
        v[0, 0, 0:128:2, 1] = 1.0
        assert slabs_differ(c.volume_download(0, shape), v) is None
