"""CPU side of mask morphology (vr_mask_morph, include/vr.h): the restatement the GPU tests compare against (morph_ref.py) pinned to
scipy.ndimage and to the algebra's laws; the two host fillers vr_morph_ball / vr_morph_box, called through the binding with no context,
against an int64 restatement; the struct layouts against the header; the random sweep's generator."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import morph_cases as mc
import morph_ref as mr
from volumerendering_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
SHAPE = (21, 37, 70)  # (nz, ny, nx): the issue's 70 x 37 x 21


def test_constants_match_the_binding():
    assert (mr.NONE, mr.DILATE, mr.ERODE, mr.CLOSE, mr.OPEN) == (capi.MORPH_NONE, capi.MORPH_DILATE, capi.MORPH_ERODE, capi.MORPH_CLOSE, capi.MORPH_OPEN)
    assert (mr.REPLACE, mr.OR, mr.AND, mr.ANDNOT) == (capi.MORPH_REPLACE, capi.MORPH_OR, capi.MORPH_AND, capi.MORPH_ANDNOT)
    assert mr.MAX_RADIUS == capi.MORPH_MAX_RADIUS == 31


# ---- the fillers (these fail where the library lacks the symbols) --------------------------------------------------------------------

def same_element(e: capi.MorphElement, want):
    radii, half = mc.from_capi(e)
    table = np.ctypeslib.as_array(e.half)
    outside = table.copy()
    outside[:half.shape[0], :half.shape[1]] = -1
    return radii == want[0] and np.array_equal(half, want[1]) and (outside == -1).all()


@pytest.mark.parametrize("spacing,radius", mc.BALLS)
def test_morph_ball_equals_the_int64_restatement(spacing, radius):
    e = capi.morph_ball(spacing, radius)
    want = mr.ball(spacing, radius)
    assert same_element(e, want) and mr.valid(mc.from_capi(e))
    if (spacing, radius) == mc.REACH:
        assert want[0] == (31, 22, 17) and int(want[1].max()) == 31


def test_morph_ball_random_inputs():
    inputs = mc.ball_inputs(200)
    assert any(max(sp) == 1 << 20 for sp, _ in inputs) and any(r // min(sp) == 31 for sp, r in inputs)
    for sp, radius in inputs:
        assert all(radius // s <= 31 for s in sp)
        e = capi.morph_ball(sp, radius)
        want = mr.ball(sp, radius)
        assert same_element(e, want), (sp, radius)
        assert mr.valid(want), (sp, radius)  # symmetric, holds the origin, every entry in -1 .. rx


def test_unit_ball_is_the_six_neighbour_cross_and_boxes_are_full():
    radii, half = mc.from_capi(capi.morph_ball((1, 1, 1), 1))
    assert radii == (1, 1, 1) and half.tolist() == [[-1, 0, -1], [0, 1, 0], [-1, 0, -1]]
    s = mr.structure((radii, half))
    assert int(s.sum()) == 7 and s[1, 1, :].all() and s[1, :, 1].all() and s[:, 1, 1].all()
    assert same_element(capi.morph_box(1, 1, 0), mr.box(1, 1, 0)) and mr.structure(mr.box(1, 1, 0)).shape == (1, 3, 3)
    assert same_element(capi.morph_box(31, 0, 31), mr.box(31, 0, 31)) and same_element(capi.morph_box(0, 0, 0), mr.box(0, 0, 0))
    assert mr.structure(mr.box(2, 3, 4)).all()


def test_filler_errors():
    lib = capi.load()
    e = capi.MorphElement()
    sp = lambda *s: C.byref((C.c_uint32 * 3)(*s))  # noqa: E731
    assert lib.vr_morph_ball(sp(1000, 1000, 3000), 5000, C.byref(e)) == capi.VR_OK
    for bad in ((0, 1, 1), (1, 0, 1), (1, 1, 0), ((1 << 20) + 1, 1, 1)):
        assert lib.vr_morph_ball(sp(*bad), 5, C.byref(e)) == capi.VR_ERR_INVALID_ARG, bad
    assert lib.vr_morph_ball(sp(1 << 20, 1 << 20, 1 << 20), 31 << 20, C.byref(e)) == capi.VR_OK
    assert lib.vr_morph_ball(sp(100, 100, 100), 3199, C.byref(e)) == capi.VR_OK            # quotient 31
    for bad in ((100, 1000, 1000), (1000, 100, 1000), (1000, 1000, 100)):
        assert lib.vr_morph_ball(sp(*bad), 3200, C.byref(e)) == capi.VR_ERR_INVALID_ARG     # quotient 32 on one axis
    assert lib.vr_morph_ball(sp(1, 1, 1), 1, None) == capi.VR_ERR_INVALID_ARG
    assert lib.vr_morph_ball(None, 1, C.byref(e)) == capi.VR_ERR_INVALID_ARG
    for bad in ((-1, 0, 0), (0, 32, 0), (0, 0, 32), (32, 0, 0)):
        assert lib.vr_morph_box(*bad, C.byref(e)) == capi.VR_ERR_INVALID_ARG
    assert lib.vr_morph_box(1, 1, 1, None) == capi.VR_ERR_INVALID_ARG
    with pytest.raises(capi.VrError):
        capi.morph_ball((1, 1, 1), 32)


# ---- the restatement ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def sets():
    return {"sparse": mc.sparse(SHAPE), "dense": mc.dense(SHAPE)}


GOLDEN = os.path.join(ROOT, "tests", "golden", "morph_scipy_reach.npz")


def scipy_pair(ndi, b, element):
    s = mr.structure(element)
    return ndi.binary_dilation(b, structure=s, border_value=0), ndi.binary_erosion(b, structure=s, border_value=1)


def write_reach_golden():
    """Records scipy's dilation and erosion of the two sets by the ball of radii (31, 22, 17): scipy.ndimage needs a minute per call for
    that structure (49497 offsets on 54390 voxels), so the suite compares with this record; VR_MORPH_SCIPY_LIVE=1 runs scipy itself."""
    import scipy.ndimage as ndi
    out = {}
    for name, a in (("sparse", mc.sparse(SHAPE)), ("dense", mc.dense(SHAPE))):
        d, e = scipy_pair(ndi, a, mr.ball(*mc.REACH))
        out[name + "_input"], out[name + "_dilation"], out[name + "_erosion"] = np.packbits(a), np.packbits(d), np.packbits(e)
    np.savez_compressed(GOLDEN, **out)


@pytest.mark.parametrize("spacing,radius", mc.BALLS)
def test_restatement_equals_scipy(sets, spacing, radius):
    """Dilation and erosion by the chord-table formulation equal scipy.ndimage.binary_dilation(structure=S, border_value=0) and
    binary_erosion(structure=S, border_value=1) on the 70 x 37 x 21 volume and on a crop of it, and closing is extensive.  For the
    largest ball scipy's answers on the whole volume are read from tests/golden/morph_scipy_reach.npz (write_reach_golden)."""
    ndi = pytest.importorskip("scipy.ndimage")
    element = mr.ball(spacing, radius)
    recorded = np.load(GOLDEN) if (spacing, radius) == mc.REACH and not os.environ.get("VR_MORPH_SCIPY_LIVE") else None
    for name, a in sets.items():
        for crop in ((slice(None),) * 3, (slice(2, 19), slice(5, 30), slice(3, 66))):
            b = a[crop]
            if recorded is None:
                dilation, erosion = scipy_pair(ndi, b, element)
            elif crop[0] == slice(None):
                assert np.array_equal(np.packbits(b), recorded[name + "_input"])  # (the record is of this very set)
                dilation, erosion = (np.unpackbits(recorded[name + k])[:b.size].reshape(b.shape).astype(bool) for k in ("_dilation", "_erosion"))
            else:
                continue
            assert np.array_equal(mr.dilate(b, element), dilation), (name, crop)
            assert np.array_equal(mr.erode(b, element), erosion), (name, crop)
            closed = mr.apply(mr.CLOSE, b, element)
            assert (closed | ~b).all(), (name, crop)  # extensive


@pytest.mark.parametrize("element", [mr.ball(*mc.BALLS[0]), mr.ball((1, 1, 1), 1), mr.ball((1, 1, 1), 5), mr.box(1, 1, 0), mr.box(0, 0, 3), mr.box(3, 2, 1)],
                         ids=["ball5mm", "cross", "ball5", "box110", "box003", "box321"])
def test_laws_of_the_operators(sets, element):
    for name, a in sets.items():
        opened, closed = mr.apply(mr.OPEN, a, element), mr.apply(mr.CLOSE, a, element)
        assert np.array_equal(mr.apply(mr.OPEN, opened, element), opened), name     # idempotent
        assert np.array_equal(mr.apply(mr.CLOSE, closed, element), closed), name
        assert (closed | ~a).all() and (a | ~opened).all(), name                    # A in close(A), open(A) in A
        assert (mr.dilate(a, element) | ~a).all() and (a | ~mr.erode(a, element)).all()
    assert mr.erode(np.ones(SHAPE, bool), element).all()  # the outside of the box does not erode
    assert not mr.dilate(np.zeros(SHAPE, bool), element).any()


def test_dilation_is_cut_at_the_box():
    """dilate(A) of a box equals the box's part of the dilation in a volume large enough that nothing is cut."""
    element = mr.ball(*mc.BALLS[0])
    rx, ry, rz = element[0]
    a = mc.dense(SHAPE, seed=9)
    big = np.zeros((SHAPE[0] + 2 * rz, SHAPE[1] + 2 * ry, SHAPE[2] + 2 * rx), bool)
    big[rz:-rz, ry:-ry, rx:-rx] = a
    assert np.array_equal(mr.dilate(a, element), mr.dilate(big, element)[rz:-rz, ry:-ry, rx:-rx])
    # through morph: a box inside the volume, set voxels outside it are not read, voxels outside it are not written
    v = np.zeros(SHAPE + (4,), f32)
    v[..., 1] = a
    lo, hi = (3, 5, 2), (66, 30, 19)
    out, n, n_src, bb, nbox, r = mr.morph(v, v, 1, 1, mr.DILATE, mr.REPLACE, lo, hi, element)
    crop = (slice(2, 19), slice(5, 30), slice(3, 66))
    assert np.array_equal(r[crop], mr.dilate(a[crop], element)) and int(r.sum()) == n == int(r[crop].sum())
    outside = np.ones(SHAPE, bool)
    outside[crop] = False
    assert np.array_equal(out[..., 1][outside], v[..., 1][outside]) and n_src == int(a[crop].sum()) and nbox == 63 * 25 * 17


def test_combine_modes_on_bit_patterns():
    a = np.array([[[1, 0, 1, 0, 1, 0]]], bool)
    src = np.zeros((1, 1, 6, 4), f32)
    src[..., 0] = np.array([np.nan, -0.0, 2.5, 0.0, 1.0, -0.0], f32)
    assert np.array_equal(mr.member(src[..., 0]), a)
    dst = mc.arbitrary_bits((1, 1, 6), seed=5).copy()
    cur = np.array([0x7FC00001, 0x80000000, 0x00000000, 0xFFC12345, 0x3F800000, 0x40200000], np.uint32)
    dst[..., 2] = cur.view(f32)
    one = 0x3F800000
    want = {mr.REPLACE: [one, 0, one, 0, one, 0], mr.OR: [one, cur[1], one, cur[3], one, cur[5]],
            mr.AND: [cur[0], 0, cur[2], 0, cur[4], 0], mr.ANDNOT: [0, cur[1], 0, cur[3], 0, cur[5]]}
    for combine, bits in want.items():
        out, n, n_src, bb, nbox, r = mr.morph(src, dst, 0, 2, mr.NONE, combine, (0, 0, 0), (6, 1, 1), None)
        assert out[..., 2].view(np.uint32).ravel().tolist() == [int(b) for b in bits], combine
        keep = [0, 1, 3]
        assert np.array_equal(out[..., keep].view(np.uint32), dst[..., keep].view(np.uint32))
        assert (n, n_src, bb, nbox) == (3, 3, ((0, 0, 0), (5, 1, 1)), 6)
    # an empty destination slot is created zeroed; an empty box changes nothing and reports zeros
    out = mr.morph(src, None, 0, 3, mr.NONE, mr.OR, (0, 0, 0), (6, 1, 1), None)[0]
    assert out[..., 3].ravel().tolist() == [1, 0, 1, 0, 1, 0] and not out[..., :3].view(np.uint32).any()
    out, n, n_src, bb, nbox, r = mr.morph(src, dst, 0, 2, mr.DILATE, mr.REPLACE, (2, 0, 0), (2, 1, 1), mr.box(1, 0, 0))
    assert np.array_equal(out.view(np.uint32), dst.view(np.uint32)) and (n, n_src, bb, nbox) == (0, 0, ((0, 0, 0), (0, 0, 0)), 0)


def test_sweep_generator_gives_valid_descriptors():
    cases = mc.sweep(40)
    assert len(cases) == 40
    for c in cases:
        nz, ny, nx = c["shape"]
        assert all(1 <= n <= 140 for n in c["shape"])
        assert all(0 <= l <= h <= n for l, h, n in zip(c["box_lo"], c["box_hi"], (nx, ny, nz))), c
        assert mr.valid(c["element"]) and all(r <= n for r, n in zip(c["element"][0], (nx, ny, nz))), c
        assert c["op"] in range(5) and c["combine"] in range(4) and c["src_contour"] in range(4) and c["dst_contour"] in range(4)
        assert c["src_slot"] in range(capi.MAX_VOLUMES) and c["dst_slot"] in range(capi.MAX_VOLUMES)
        assert same_element(mc.to_capi(c["element"]), c["element"])
    # the sweep covers every operator, every way of storing, both kinds of element, in-place and fresh destinations
    assert {c["op"] for c in cases} == set(range(5)) and {c["combine"] for c in cases} == set(range(4))
    assert any(c["fresh"] for c in cases) and any(c["src_slot"] == c["dst_slot"] and c["src_contour"] == c["dst_contour"] for c in cases)
    assert sum(60 <= c["shape"][2] <= 70 for c in cases) >= 8 and sum(125 <= c["shape"][2] <= 135 for c in cases) >= 8


# ---- the binding -----------------------------------------------------------------------------------------------------------------------

def test_morph_struct_layouts_match_header(tmp_path):
    fields_e = ["radius", "half"]
    fields_d = ["src_slot", "src_contour", "dst_slot", "dst_contour", "op", "combine", "box_lo", "box_hi", "element"]
    fields_r = ["voxels", "src_voxels", "lo", "hi"]
    args = ["sizeof(vr_morph_element)"] + [f"offsetof(vr_morph_element, {f})" for f in fields_e]
    args += ["sizeof(vr_morph_desc)"] + [f"offsetof(vr_morph_desc, {f})" for f in fields_d]
    args += ["sizeof(vr_morph_result)"] + [f"offsetof(vr_morph_result, {f})" for f in fields_r]
    consts = ["VR_MORPH_MAX_RADIUS", "VR_MORPH_NONE", "VR_MORPH_DILATE", "VR_MORPH_ERODE", "VR_MORPH_CLOSE", "VR_MORPH_OPEN",
              "VR_MORPH_REPLACE", "VR_MORPH_OR", "VR_MORPH_AND", "VR_MORPH_ANDNOT", "VR_ABI_VERSION"]
    args += [f"(size_t){c}" for c in consts]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vr.h"\nint main(){' +
                   "".join(f'printf("%zu ", {a});' for a in args) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    E, D, R = capi.MorphElement, capi.MorphDesc, capi.MorphResult
    want = [C.sizeof(E)] + [getattr(E, f).offset for f in fields_e] + [C.sizeof(D)] + [getattr(D, f).offset for f in fields_d]
    want += [C.sizeof(R)] + [getattr(R, f).offset for f in fields_r]
    want += [capi.MORPH_MAX_RADIUS, capi.MORPH_NONE, capi.MORPH_DILATE, capi.MORPH_ERODE, capi.MORPH_CLOSE, capi.MORPH_OPEN,
             capi.MORPH_REPLACE, capi.MORPH_OR, capi.MORPH_AND, capi.MORPH_ANDNOT, 1]
    assert out == want
    assert C.sizeof(E) == 12 + 63 * 63 + 3 and C.sizeof(D) == 48 + C.sizeof(E) and C.sizeof(R) == 40


def test_morph_desc_copy():
    d = capi.MorphDesc()
    ball = mc.to_capi(mr.ball((1, 1, 1), 5))
    e = d.copy(src_slot=2, op=capi.MORPH_CLOSE, box_hi=(3, 4, 5), element=ball)
    assert (e.src_slot, e.op, list(e.box_hi), list(e.box_lo)) == (2, capi.MORPH_CLOSE, [3, 4, 5], [0, 0, 0])
    assert list(e.element.radius) == [5, 5, 5] and e.element.half[5][5] == 5 and d.op == 0 and list(d.element.radius) == [0, 0, 0]
    ball.half[5][5] = 0  # (the copy holds its own element)
    assert e.element.half[5][5] == 5 and e.copy(combine=capi.MORPH_ANDNOT).combine == capi.MORPH_ANDNOT
    assert bytes(e.copy()) == bytes(e)
