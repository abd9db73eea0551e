"""CPU side of the distance maps (vr_mask_distance, include/vr.h): the restatement the GPU tests compare against (dist_ref.py) pinned to
scipy.ndimage.distance_transform_edt, to the definition itself and to the two laws that tie it to the morphology (morph_ref.py); why
equality of the stored f32 channel proves equality of the squared distances on the shapes the GPU tests use; the constants and the
struct layouts against the header; the filler through the binding with no device; the random sweep's generator."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import dist_cases as dc
import dist_ref as dr
import morph_ref as mr
from volumerendering_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
SHAPE = (21, 37, 70)  # (nz, ny, nx)


# ---- the binding (these fail where the header, the binding or the library lack the feature) ------------------------------------------

def test_constants_and_struct_layouts_match_header(tmp_path):
    fields_d = ["src_slot", "src_contour", "dst_slot", "dst_channel", "mode", "probe_slot", "probe_contour", "limit", "spacing", "scale",
                "box_lo", "box_hi"]
    fields_r = ["src_voxels", "lo", "hi", "beyond", "probe_voxels", "probe_min_sq", "probe_max_sq"]
    args = ["sizeof(vr_dist_desc)"] + [f"offsetof(vr_dist_desc, {f})" for f in fields_d]
    args += ["sizeof(vr_dist_result)"] + [f"offsetof(vr_dist_result, {f})" for f in fields_r]
    args += [f"(size_t){c}" for c in ("VR_DIST_OUTSIDE", "VR_DIST_INSIDE", "VR_DIST_SIGNED", "VR_ABI_VERSION")]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vr.h"\nint main(){' +
                   "".join(f'printf("%zu ", {a});' for a in args) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    D, R = capi.DistDesc, capi.DistResult
    want = [C.sizeof(D)] + [getattr(D, f).offset for f in fields_d] + [C.sizeof(R)] + [getattr(R, f).offset for f in fields_r]
    want += [capi.DIST_OUTSIDE, capi.DIST_INSIDE, capi.DIST_SIGNED, 1]
    assert out == want
    assert C.sizeof(D) == 72 and C.sizeof(R) == 64
    assert (dr.OUTSIDE, dr.INSIDE, dr.SIGNED) == (capi.DIST_OUTSIDE, capi.DIST_INSIDE, capi.DIST_SIGNED) == (0, 1, 2)
    assert (dr.MAX_SPACING, dr.MAX_LIMIT, dr.MAX_EXTENT) == (capi.DIST_MAX_SPACING, capi.DIST_MAX_LIMIT, capi.DIST_MAX_EXTENT) == (1 << 20, 1 << 31, 1 << 30)


def test_dist_whole_without_a_device():
    """The filler is host arithmetic: without a context or an output it is VR_ERR_INVALID_ARG, whatever the other arguments."""
    lib = capi.load()
    d = capi.DistDesc()
    assert lib.vr_dist_whole(None, 0, 0, 1, 3, capi.DIST_SIGNED, None) == capi.VR_ERR_INVALID_ARG
    assert lib.vr_dist_whole(None, 0, 0, 1, 3, capi.DIST_SIGNED, C.byref(d)) == capi.VR_ERR_INVALID_ARG
    assert lib.vr_mask_distance(None, C.byref(d), None) == capi.VR_ERR_INVALID_ARG
    assert lib.vr_dist_counters(None, None) == capi.VR_ERR_INVALID_ARG and lib.vr_dist_timing(None, None) == capi.VR_ERR_INVALID_ARG
    for name in ("vr_dist_whole", "vr_mask_distance", "vr_dist_counters", "vr_dist_timing"):
        assert name in capi.ABI_SYMBOLS


def test_dist_desc_copy():
    d = capi.DistDesc()
    e = d.copy(src_slot=2, mode=capi.DIST_SIGNED, box_hi=(3, 4, 5), spacing=(1000, 1000, 3000), limit=20000, scale=0.001, probe_slot=-1)
    assert (e.src_slot, e.mode, list(e.box_hi), list(e.box_lo), list(e.spacing), e.limit, e.probe_slot) == (2, 2, [3, 4, 5], [0, 0, 0], [1000, 1000, 3000], 20000, -1)
    assert f32(e.scale) == f32(0.001) and d.mode == 0 and list(d.spacing) == [0, 0, 0] and bytes(e.copy()) == bytes(e)


# ---- the restatement -------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def sets():
    return {"sparse": dc.sparse(SHAPE), "dense": dc.dense(SHAPE), "shell": dc.shell(SHAPE)}


@pytest.mark.parametrize("spacing", [dc.UNIT, dc.MM, (2, 3, 5), (977, 977, 2500)], ids=["unit", "1x1x3mm", "2x3x5", "ct"])
def test_restatement_equals_scipy(sets, spacing):
    """round(edt^2) == D2: scipy's distance_transform_edt(sampling) is the double-precision square root of the exact squared distance
    (below 2^53 here), of the background to the set for D2out and of the set to the background for D2in."""
    ndi = pytest.importorskip("scipy.ndimage")
    for name, a in sets.items():
        for crop in ((slice(None),) * 3, (slice(2, 19), slice(5, 30), slice(3, 66))):
            b = a[crop]
            d2out, d2in = dr.fields(b, spacing)
            sampling = tuple(float(s) for s in spacing[::-1])  # (z, y, x)
            assert np.array_equal(np.rint(ndi.distance_transform_edt(~b, sampling=sampling) ** 2).astype(np.int64), d2out), (name, crop)
            assert np.array_equal(np.rint(ndi.distance_transform_edt(b, sampling=sampling) ** 2).astype(np.int64), d2in), (name, crop)
            assert (d2out[b] == 0).all() and (d2out[~b] > 0).all() and (d2in[~b] == 0).all() and (d2in[b] > 0).all()


def test_restatement_equals_the_definition():
    """The separable passes equal the minimum over the set voxels taken directly, also at the largest spacing, 2^20."""
    shape = (5, 7, 11)
    pts = [(0, 0, 0), (10, 6, 4), (3, 2, 1), (7, 5, 2)]
    a = dc.points(shape, pts)
    for spacing in (dc.UNIT, (1 << 20, 1 << 20, 1 << 20), (95325, 1 << 20, 3)):
        assert dr.legal(*dc.whole(shape), spacing)
        assert np.array_equal(dr.d2_field(a, spacing), dr.d2_from_points(shape, pts, spacing)), spacing
    assert (dr.d2_field(np.zeros(shape, bool), dc.UNIT) == dr.BEYOND).all()
    assert int(dr.d2_field(a, (1 << 20,) * 3).max()) > 1 << 45


@pytest.mark.parametrize("spacing,radius", [(dc.MM, 5000), ((977, 977, 2500), 7000), (dc.UNIT, 1), (dc.UNIT, 5), ((500, 700, 900), 15500)])
def test_the_two_morph_laws(sets, spacing, radius):
    """{p : D2out(p) <= r^2} is the dilation by the ball of vr_morph_ball(spacing, r), {p in box : D2in(p) > r^2} the erosion by it."""
    element = mr.ball(spacing, radius)
    for name, a in sets.items():
        d2out, d2in = dr.fields(a, spacing)
        assert np.array_equal(d2out <= radius ** 2, mr.dilate(a, element)), name
        assert np.array_equal(d2in > radius ** 2, mr.erode(a, element)), name
    full = np.ones(SHAPE, bool)
    assert (dr.d2_field(~full, spacing) == dr.BEYOND).all() and mr.erode(full, element).all()  # (the outside of the box does not erode)


def test_channel_equality_proves_field_equality():
    """INJECTIVITY.  On the unit-spacing shapes the GPU tests use, D2 <= sum (n_a - 1)^2 < 2^24, so (float)D2 is exact, and the correctly
    rounded f32 square roots of distinct integers below that bound are distinct (neighbouring roots are 1 / (2 sqrt(D2)) >= 0.0036 apart,
    an ulp there is at most 2^-16): two fields that store the same channel are the same fields.  Multiplying by a scale of 1 keeps that."""
    top = max(sum((n - 1) ** 2 for n in shape) for shape in dc.UNIT_SHAPES + [c["shape"] for c in dc.sweep(40)])
    assert top < 1 << 24
    d2 = np.arange(top + 1, dtype=np.int64)
    m = dr.magnitude(d2, 0, 1.0)
    assert m.dtype == np.float32 and (np.diff(m) > 0).all()
    assert np.array_equal(d2.astype(np.float32).astype(np.int64), d2)


def test_stored_values_modes_limit_and_probe():
    a = np.array([[[0, 0, 1, 1, 0, 0, 0, 0]]], bool)
    src = np.zeros((1, 1, 8, 4), f32)
    src[..., 1] = np.array([-0.0, 0.0, np.nan, 2.5, 0.0, -0.0, 0.0, 0.0], f32)
    assert np.array_equal(dr.member(src[..., 1]), a)
    dst = dc.arbitrary_bits((1, 1, 8), seed=5)
    box = ((0, 0, 0), (8, 1, 1))
    probe = np.zeros((1, 1, 8, 4), f32)
    probe[0, 0, [3, 5, 7], 2] = 1.0
    sp = (1000, 1, 1)
    out, res, nbox = dr.distance(src, dst, 1, 3, dr.OUTSIDE, *box, sp, 0, 0.001, probe, 2)
    assert np.array_equal(out[..., 3].ravel(), np.array([2000, 1000, 0, 0, 1000, 2000, 3000, 4000], f32) * f32(0.001)) and nbox == 8
    assert res == (2, (2, 0, 0), (4, 1, 1), 0, 3, 0, 16000000)
    assert np.array_equal(out[..., :3].view(np.uint32), dst[..., :3].view(np.uint32))
    out, res, _ = dr.distance(src, dst, 1, 3, dr.INSIDE, *box, sp, 0, 0.001)
    assert out[..., 3].ravel().tolist() == [0.0, 0.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0] and res[3] == 0
    out, res, _ = dr.distance(src, dst, 1, 3, dr.SIGNED, *box, sp, 2000, 0.001, probe, 2)
    assert out[..., 3].ravel().tolist() == [2.0, 1.0, -1.0, -1.0, 1.0, 2.0, 2.0, 2.0] and not (out[..., 3] == 0).any()
    assert res == (2, (2, 0, 0), (4, 1, 1), 2, 3, 0, dr.U64_MAX)  # (x = 6 and 7 are beyond 2 mm; a value equal to the limit is not)
    # an empty set: +inf without a limit, the limit with one; a box of part of the row; a fresh destination
    none = np.zeros_like(src)
    out, res, _ = dr.distance(none, None, 1, 0, dr.SIGNED, (1, 0, 0), (6, 1, 1), sp, 0, 1.0, probe, 2)
    assert np.isposinf(out[0, 0, 1:6, 0]).all() and not out[0, 0, [0, 6, 7], 0].any() and res == (0, (0, 0, 0), (0, 0, 0), 5, 2, dr.U64_MAX, dr.U64_MAX)
    out, res, _ = dr.distance(none, None, 1, 0, dr.OUTSIDE, (1, 0, 0), (6, 1, 1), sp, 7, 0.5)
    assert (out[0, 0, 1:6, 0] == 3.5).all() and res[3] == 5
    full = np.ones_like(src)
    out, res, _ = dr.distance(full, None, 1, 0, dr.SIGNED, (1, 0, 0), (6, 1, 1), sp, 0, 1.0)
    assert np.isneginf(out[0, 0, 1:6, 0]).all() and res[0] == 5 and res[3] == 5  # (the outside of the box is not background)
    out, res, nbox = dr.distance(src, dst, 1, 3, dr.SIGNED, (2, 0, 0), (2, 1, 1), sp)
    assert np.array_equal(out.view(np.uint32), dst.view(np.uint32)) and res == (0, (0, 0, 0), (0, 0, 0), 0, 0, 0, 0) and nbox == 0


def test_legal_extents():
    assert dr.legal((0, 0, 0), (65535, 1, 2), (16384, 1, 1)) and not dr.legal((0, 0, 0), (65535, 1, 2), (16385, 1, 1))
    assert dr.legal((10, 0, 0), (65535, 1, 2), (16386, 1, 1)) and not dr.legal((0, 0, 0), (4, 4, 4), (1, 0, 1))
    assert not dr.legal((0, 0, 0), (4, 4, 4), (1, (1 << 20) + 1, 1)) and dr.legal((0, 0, 0), (4, 4, 4), (1, 1, 1), 1 << 31)
    assert not dr.legal((0, 0, 0), (4, 4, 4), (1, 1, 1), (1 << 31) + 1)


def test_sweep_generator_gives_valid_descriptors():
    cases = dc.sweep(40)
    assert len(cases) == 40
    for c in cases:
        nz, ny, nx = c["shape"]
        assert 1 <= nx <= 130 and 1 <= ny <= 37 and 1 <= nz <= 21
        assert all(0 <= l <= h <= n for l, h, n in zip(c["box_lo"], c["box_hi"], (nx, ny, nz))), c
        assert dr.legal(c["box_lo"], c["box_hi"], c["spacing"], c["limit"]) and c["scale"] > 0
        assert c["mode"] in range(3) and c["src_contour"] in range(4) and c["dst_channel"] in range(4)
        assert c["probe"] is None or (c["probe"] in range(4) and c["mode"] != dr.INSIDE)
    assert {c["mode"] for c in cases} == set(range(3)) and {c["layout"] for c in cases} == {0, 1, 3}
    assert any(c["fresh"] for c in cases) and any(c["src_slot"] == c["dst_slot"] for c in cases)
    assert any(c["limit"] for c in cases) and any(not c["limit"] for c in cases) and any(c["probe"] is not None for c in cases)
    assert sum(c["shape"][2] > 64 for c in cases) >= 8
