"""CPU side of the resampling tool (vr_volume_resample, include/vr.h): the constants and struct layouts against the header, the fillers
through the binding with no device, vr_resample_between against its float64 restatement exactly, the identity law and the settling
argument on the restatement the GPU tests compare against (resample_ref.py), and that the GPU tests' cases are what they are meant
to be."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import proj_ref as pr
import resample_cases as rc
import resample_ref as rr
from volumerendering_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


# ---- the binding (these fail where the header, the binding or the library lack the feature) ------------------------------------------

def test_constants_and_struct_layouts_match_header(tmp_path):
    fields_d = ["src_slot", "dst_slot", "channels", "filter", "dst_n", "origin", "di", "dj", "dk", "outside", "box_lo", "box_hi"]
    fields_r = ["inside", "outside", "lo", "hi"]
    fields_g = ["n", "origin", "spacing"]
    args = ["sizeof(vr_resample_desc)"] + [f"offsetof(vr_resample_desc, {f})" for f in fields_d]
    args += ["sizeof(vr_resample_result)"] + [f"offsetof(vr_resample_result, {f})" for f in fields_r]
    args += ["sizeof(vr_grid)"] + [f"offsetof(vr_grid, {f})" for f in fields_g]
    args += [f"(size_t){c}" for c in ("VR_RESAMPLE_LINEAR", "VR_RESAMPLE_NEAREST", "VR_ABI_VERSION")]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vr.h"\nint main(){' +
                   "".join(f'printf("%zu ", {a});' for a in args) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    D, R, G = capi.ResampleDesc, capi.ResampleResult, capi.Grid
    want = [C.sizeof(D)] + [getattr(D, f).offset for f in fields_d] + [C.sizeof(R)] + [getattr(R, f).offset for f in fields_r]
    want += [C.sizeof(G)] + [getattr(G, f).offset for f in fields_g] + [capi.RESAMPLE_LINEAR, capi.RESAMPLE_NEAREST, 1]
    assert out == want
    assert (C.sizeof(D), C.sizeof(R), C.sizeof(G)) == (116, 40, 64)
    assert (rr.LINEAR, rr.NEAREST) == (capi.RESAMPLE_LINEAR, capi.RESAMPLE_NEAREST) == (0, 1)


def test_entry_points_without_a_device():
    """Every entry point refuses a NULL context or output with VR_ERR_INVALID_ARG; vr_resample_between is host arithmetic and works."""
    lib = capi.load()
    d = capi.ResampleDesc()
    assert lib.vr_resample_identity(None, 0, 1, 0, C.byref(d)) == capi.VR_ERR_INVALID_ARG
    assert lib.vr_resample_identity(None, 0, 1, 0, None) == capi.VR_ERR_INVALID_ARG
    assert lib.vr_volume_resample(None, C.byref(d), None) == capi.VR_ERR_INVALID_ARG
    assert lib.vr_resample_counters(None, None) == capi.VR_ERR_INVALID_ARG and lib.vr_resample_timing(None, None) == capi.VR_ERR_INVALID_ARG
    g = capi.Grid.of((4, 5, 6), (0, 0, 0), (1, 1, 1))
    assert lib.vr_resample_between(None, C.byref(g), None, C.byref(d)) == capi.VR_ERR_INVALID_ARG
    assert lib.vr_resample_between(C.byref(g), None, None, C.byref(d)) == capi.VR_ERR_INVALID_ARG
    assert lib.vr_resample_between(C.byref(g), C.byref(g), None, None) == capi.VR_ERR_INVALID_ARG
    assert lib.vr_resample_between(C.byref(g), C.byref(g), None, C.byref(d)) == capi.VR_OK
    for name in ("vr_resample_identity", "vr_resample_between", "vr_volume_resample", "vr_resample_counters", "vr_resample_timing"):
        assert name in capi.ABI_SYMBOLS and hasattr(lib, name)


def test_resample_desc_copy():
    d = capi.ResampleDesc()
    e = d.copy(src_slot=2, dst_slot=1, channels=8, filter=1, dst_n=(3, 4, 5), origin=(0.5, 0.25, 0.125), dk=(0, 0, 1), outside=(1, 2, 3, 4),
               box_hi=(3, 4, 5))
    assert (e.src_slot, e.dst_slot, e.channels, e.filter, list(e.dst_n), list(e.box_lo), list(e.box_hi)) == (2, 1, 8, 1, [3, 4, 5], [0, 0, 0], [3, 4, 5])
    assert list(e.origin) == [0.5, 0.25, 0.125] and list(e.dk) == [0, 0, 1] and list(e.di) == [0, 0, 0] and list(e.outside) == [1, 2, 3, 4]
    assert d.channels == 0 and bytes(e.copy()) == bytes(e)


# ---- vr_resample_between ---------------------------------------------------------------------------------------------------------------

def dose_in_ct():
    """C4's geometry: a 128 x 128 x 64 dose of 2.5 x 2.5 x 3 mm inside a 512^3 CT of 0.977 x 0.977 x 1.25 mm, offset by fractions."""
    ct = ((512, 512, 512), (-250.1, -249.7, -310.0), (0.977, 0.977, 1.25))
    dose = ((128, 128, 64), (-161.3, -158.9, -97.25), (2.5, 2.5, 3.0))
    return ct, dose


BETWEEN = {
    "dose onto ct": lambda: (dose_in_ct()[1], dose_in_ct()[0], None),
    "ct onto dose": lambda: (dose_in_ct()[0], dose_in_ct()[1], None),
    "anisotropic": lambda: (((70, 9, 5), (1e-3, -7.25, 1234.5), (0.31, 1.7, 5.0)), ((130, 6, 7), (3.3, 0.1, -9.9), (0.123456789, 2.2, 0.7)), None),
    "rotation": lambda: rc.grids("oblique", (5, 9, 70), (7, 6, 130)),
    "rotation z": lambda: rc.grids("rot30z", (6, 7, 1), (2, 1, 65)),
    "general affine": lambda: (((65535, 1, 2), (0, 0, 0), (1e-3, 1e3, 1.0)), ((1, 65535, 3), (1e6, -1e6, 0.5), (7.0, 1e-2, 3.0)),
                               np.array([[0.1, -2.0, 3.5, 100.0], [1e-3, 0.0, -1.0, -3.25], [7.0, 7.0, 7.0, 1e5]])),
}


@pytest.mark.parametrize("name", list(BETWEEN))
def test_between_equals_the_float64_restatement_exactly(name):
    src, dst, m = BETWEEN[name]()
    d = capi.resample_between(capi.Grid.of(*src), capi.Grid.of(*dst), m)
    want = rr.between(*src, *dst, m)
    for got, w in zip((d.origin, d.di, d.dj, d.dk), want):
        assert np.array_equal(bits(np.array(list(got), f32)), bits(w)), (name, list(got), w)
    assert list(d.dst_n) == list(dst[0]) and list(d.box_lo) == [0, 0, 0] and list(d.box_hi) == list(dst[0])
    assert (d.src_slot, d.dst_slot, d.channels, d.filter, list(d.outside)) == (0, 0, 0, 0, [0, 0, 0, 0])  # (nothing else is filled)
    if m is None:  # NULL is the identity matrix
        e = capi.resample_between(capi.Grid.of(*src), capi.Grid.of(*dst), [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0])
        assert bytes(e) == bytes(d)


def test_between_puts_voxel_centres_where_the_geometry_says():
    """One grid onto itself is the identity filler's geometry up to rounding; the dose's voxel (0, 0, 0) lands in the CT where its
    patient position says (texture coordinate (v + 0.5) / n of the CT voxel coordinate v)."""
    g = ((8, 16, 32), (1.5, -2.0, 7.0), (0.5, 2.0, 0.25))
    o, di, dj, dk = rr.between(*g, *g)
    n, io, idi, idj, idk = rr.identity((32, 16, 8))
    assert np.array_equal(o, np.array(io, f32)) and np.array_equal(di, np.array(idi, f32)) and np.array_equal(dj, np.array(idj, f32)) and np.array_equal(dk, np.array(idk, f32))
    ct, dose = dose_in_ct()
    o, di, dj, dk = rr.between(*ct, *dose)
    v = (np.array(dose[1]) - np.array(ct[1])) / np.array(ct[2])
    assert np.allclose(o, (v + 0.5) / 512.0, rtol=0, atol=1e-7)
    assert np.allclose([di[0], dj[1], dk[2]], np.array(dose[2]) / np.array(ct[2]) / 512.0, rtol=1e-6) and di[1] == di[2] == dj[0] == dk[1] == 0


def test_between_errors():
    lib = capi.load()
    good = ((4, 5, 6), (0.0, 0.0, 0.0), (1.0, 2.0, 3.0))
    d = capi.ResampleDesc()

    def rc_of(src, dst, m=None):
        mm = None if m is None else C.byref((C.c_double * 12)(*m))
        return lib.vr_resample_between(C.byref(capi.Grid.of(*src)), C.byref(capi.Grid.of(*dst)), mm, C.byref(d))

    assert rc_of(good, good) == capi.VR_OK
    for sp in ((0.0, 1, 1), (1, -1.0, 1), (1, 1, float("inf")), (float("nan"), 1, 1)):
        assert rc_of((good[0], good[1], sp), good) == capi.VR_ERR_INVALID_ARG and rc_of(good, (good[0], good[1], sp)) == capi.VR_ERR_INVALID_ARG
    for n in ((0, 5, 6), (4, 65536, 6), (4, 5, -1)):
        assert rc_of((n, good[1], good[2]), good) == capi.VR_ERR_INVALID_ARG and rc_of(good, (n, good[1], good[2])) == capi.VR_ERR_INVALID_ARG
    assert rc_of(((65535, 1, 65535), good[1], good[2]), ((1, 65535, 1), good[1], good[2])) == capi.VR_OK
    eye = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]
    for i in range(12):
        for bad in (float("nan"), float("inf"), float("-inf")):
            assert rc_of(good, good, eye[:i] + [bad] + eye[i + 1:]) == capi.VR_ERR_INVALID_ARG
    with pytest.raises(capi.VrError):
        capi.resample_between(capi.Grid.of(*good), capi.Grid.of(good[0], good[1], (0, 1, 1)))
    # no value of an origin is an error: it only moves the grid
    assert rc_of((good[0], (float("nan"), 0, 1e300), good[2]), good) == capi.VR_OK


# ---- the restatement -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fused", [False, True], ids=["separate", "fused"])
@pytest.mark.parametrize("filt", [rr.LINEAR, rr.NEAREST], ids=["linear", "nearest"])
def test_identity_law(filt, fused):
    """THE IDENTITY LAW.  With power-of-two dimensions (8 x 16 x 32) the identity descriptor's positions (i + 0.5) / n are exact, the
    texel coordinate p * n - 0.5 is the integer i, every weight is 0 and a + (b - a) * 0 = a for finite values: the source comes back
    bit for bit, LINEAR and NEAREST, in both arithmetic modes.  With 70 x 9 x 5 it does not under LINEAR: 0.5f / 70 and i / 70 round,
    the weights are a few ulps off 0 or 1 -- with separately rounded arithmetic 38 % of the components come back equal and the rest differ
    by up to 2.2e-5 on values of unit variance (fused: 91 % equal, up to 1.8e-5).  NEAREST still returns every voxel."""
    src = rc.volume(rc.POW2, 5)
    n, o, di, dj, dk = rr.identity(rc.POW2)
    out, res, box, _ = rr.resample(src, None, n, 15, filt, o, di, dj, dk, (9, 9, 9, 9), (0, 0, 0), n, fused)
    assert np.array_equal(bits(out), bits(src)) and res == (box, 0, (0, 0, 0), n) and box == 8 * 16 * 32
    odd = (5, 9, 70)
    src = rc.volume(odd, 5)
    n, o, di, dj, dk = rr.identity(odd)
    out, res, box, _ = rr.resample(src, None, n, 15, filt, o, di, dj, dk, (9, 9, 9, 9), (0, 0, 0), n, fused)
    assert res == (box, 0, (0, 0, 0), n)
    if filt == rr.NEAREST:
        assert np.array_equal(bits(out), bits(src))
    else:  # (the weights are off by at most a few ulps of 70: far below 1e-3 of a value difference)
        assert not np.array_equal(bits(out), bits(src)) and float(np.abs(out - src).max()) < 1e-3


def test_stored_values_and_what_keeps_its_bits():
    """One row by hand: positions, the inside test at both faces, NaN, the selected components, the box, outside, the result."""
    src = np.zeros((1, 1, 4, 4), f32)
    src[0, 0, :, 3] = [1.0, 2.0, 4.0, 8.0]
    src[0, 0, :, 0] = [-1.0, -2.0, -4.0, -8.0]
    before = rc.arbitrary_bits((1, 1, 8), 3)
    # destination voxel i lies at p.x = -0.25 + i * 0.25: -0.25 (outside), 0, 0.25, ... 1.0 (inside, the far face), 1.25, 1.5 (outside)
    args = dict(origin=(-0.25, 0.5, 0.5), di=(0.25, 0, 0), dj=(0, 0, 0), dk=(0, 0, 0), outside=(7.0, 7.5, -0.0, np.inf))
    out, res, box, copied = rr.resample(src, before, (8, 1, 1), 9, rr.LINEAR, lo=(0, 0, 0), hi=(7, 1, 1), **args)
    # texel coordinate p * 4 - 0.5: -0.5, 0.5, 1.5, 2.5, 3.5 -> clamp at both edges, halves in between
    assert out[0, 0, :7, 3].tolist() == [np.inf, 1.0, 1.5, 3.0, 6.0, 8.0, np.inf] and out[0, 0, :7, 0].tolist() == [7.0, -1.0, -1.5, -3.0, -6.0, -8.0, 7.0]
    assert np.array_equal(bits(out[0, 0, :, 1:3]), bits(before[0, 0, :, 1:3])) and np.array_equal(bits(out[0, 0, 7]), bits(before[0, 0, 7]))
    assert res == (5, 2, (1, 0, 0), (6, 1, 1)) and box == 7
    assert not copied[0, 0, 1:6, 3].any() and copied[0, 0, [0, 6, 7], 3].all() and copied[..., 1:3].all()
    out, res, _, copied = rr.resample(src, None, (8, 1, 1), 8, rr.NEAREST, lo=(0, 0, 0), hi=(8, 1, 1), **args)
    assert out[0, 0, :, 3].tolist() == [np.inf, 1.0, 2.0, 4.0, 8.0, 8.0, np.inf, np.inf] and not out[..., :3].any() and copied.all()
    assert res == (5, 3, (1, 0, 0), (6, 1, 1))
    nan = dict(args, origin=(np.nan, 0.5, 0.5))
    out, res, box, _ = rr.resample(src, before, (8, 1, 1), 15, rr.LINEAR, lo=(2, 0, 0), hi=(4, 1, 1), **nan)
    assert res == (0, 2, (0, 0, 0), (0, 0, 0)) and box == 2 and np.array_equal(bits(out[0, 0, 2]), bits(np.array(args["outside"], f32)))
    out, res, box, _ = rr.resample(src, before, (8, 1, 1), 15, rr.LINEAR, lo=(2, 0, 0), hi=(2, 1, 1), **args)
    assert res == (0, 0, (0, 0, 0), (0, 0, 0)) and box == 0 and np.array_equal(bits(out), bits(before))


@pytest.mark.parametrize("fused", [False, True], ids=["separate", "fused"])
def test_the_settling_argument(fused):
    """What csrc/vr_resample.h proves about the lerps, on the restatement: over voxels of one non-zero bit pattern the sample is that
    pattern for every weight; over zeros of either sign in any mix it is +0.0f -- also over -0.0f alone."""
    rng = np.random.default_rng(8)
    p = rng.random((4000, 3)).astype(f32)
    p[:8] = [[0, 0, 0], [1, 1, 1], [0, 1, 0.5], [0.5, 0.5, 0.5], [0.125, 0.375, 0.625], [1, 0, 0], [0.0625, 0.0625, 0.0625], [0.9999999, 0.5, 0.0000001]]
    for c in (2.5, -3e-41, 4.2535296e37, -1.0000001):
        v = np.full((6, 5, 7), c, f32)
        assert (bits(pr.sample(v, p, fused)) == bits(f32(c))).all(), c
    for zeros in (np.zeros((6, 5, 7), f32), -np.zeros((6, 5, 7), f32), np.where(rng.random((6, 5, 7)) < 0.5, f32(0.0), f32(-0.0)).astype(f32)):
        assert (bits(pr.sample(zeros, p, fused)) == 0).all()
    # an infinite constant is not reproduced (inf - inf): such a brick's record is flagged and never settles
    assert np.isnan(pr.sample(np.full((3, 3, 3), np.inf, f32), p[:16], fused)).all()


# ---- the cases of the GPU tests ----------------------------------------------------------------------------------------------------------

def test_transforms_are_what_they_are_meant_to_be():
    src_shape = rc.SRC_SHAPES[0]
    src = rc.volume(src_shape, 1)
    for dst_shape in rc.DST_SHAPES:
        n = rc.n_of(dst_shape)
        for name in rc.BOTH + rc.ALL_INSIDE + rc.ALL_OUTSIDE:
            o, di, dj, dk = rc.transform(name, src_shape, dst_shape)
            for fused in (False, True):
                _, res, box, _ = rr.resample(src, None, n, 8, rr.NEAREST, o, di, dj, dk, (0, 0, 0, 0), (0, 0, 0), n, fused)
                assert res[0] + res[1] == box == n[0] * n[1] * n[2]
                assert (res[0] > 0) == (name not in rc.ALL_OUTSIDE) and (res[1] > 0) == (name not in rc.ALL_INSIDE), (name, dst_shape, res)
    for shape in rc.DST_SHAPES:
        nx, ny, nz = rc.n_of(shape)
        bx = rc.boxes(shape)
        assert all(0 <= l <= h <= m for lo, hi in bx for l, h, m in zip(lo, hi, (nx, ny, nz)))
        vox = [int(np.prod([h - l for l, h in zip(lo, hi)])) for lo, hi in bx]
        assert vox[0] == nx * ny * nz and vox[2] == 0 and vox[3] == 1 and 0 < vox[1] < vox[0]


def test_settle_source_has_every_class_of_brick():
    a = rc.settle_source()[..., 3]
    assert (bits(a[:, :, :16]) == bits(f32(2.5))).all() and (bits(a[:, :, 16:32]) == 0).all()
    mixed = bits(a[:, :, 32:48])
    assert (mixed == 0).any() and (mixed == 0x80000000).any() and np.isin(mixed, [0, 0x80000000]).all()
    assert np.isnan(a[:, :, 48:60]).sum() == 1 and np.unique(a[:, :, 60:]).size > 1000


def test_sweep_generator_gives_valid_descriptors():
    cases = rc.sweep()
    assert len(cases) == 36
    for c in cases:
        nx, ny, nz = rc.n_of(c["dst_shape"])
        assert all(0 <= l <= h <= m for l, h, m in zip(c["box_lo"], c["box_hi"], (nx, ny, nz))), c
        assert 1 <= c["channels"] <= 15 and c["filter"] in (0, 1) and c["layout"] in (0, 1, 3) and c["flavour"] in (0, 1)
        assert all(np.asarray(c[k]).dtype == f32 and np.asarray(c[k]).shape == (3,) for k in ("origin", "di", "dj", "dk"))
    assert {c["filter"] for c in cases} == {0, 1} and {c["layout"] for c in cases} == {0, 1, 3} and {c["fused"] for c in cases} == {False, True}
    assert any(c["fresh"] for c in cases) and any(not c["fresh"] for c in cases) and any(c["channels"] == 8 for c in cases)
    assert {c["name"] for c in cases} == set(rc.BOTH + rc.ALL_INSIDE + rc.ALL_OUTSIDE)
