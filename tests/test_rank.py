"""CPU side of the rank filters (vr_volume_rank; include/vr.h): the constants and struct layouts against the header, the entry points
through the binding with no device, and the restatement the GPU tests compare against (rank_ref.py) pinned bit for bit to
scipy.ndimage's rank_filter, median_filter, minimum_filter and maximum_filter."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import rank_ref as rr
from volumerendering_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, u32 = np.float32, np.uint32
MODE = {rr.CLAMP: "nearest", rr.CONSTANT: "constant"}


# ---- the binding (these fail where the header, the binding or the library lack the feature) ------------------------------------------

def test_constants_and_struct_layouts_match_header(tmp_path):
    fields_d = ["src_slot", "src_channel", "dst_slot", "dst_channel", "radius", "rank", "border", "border_value", "box_lo", "box_hi"]
    fields_r = ["stored", "nonfinite", "changed", "lo_value", "hi_value"]
    args = ["sizeof(vr_rank_desc)"] + [f"offsetof(vr_rank_desc, {f})" for f in fields_d]
    args += ["sizeof(vr_rank_result)"] + [f"offsetof(vr_rank_result, {f})" for f in fields_r]
    args += [f"(size_t)(100 + {c})" for c in ("VR_RANK_MAX_RADIUS", "VR_RANK_MIN", "VR_RANK_MEDIAN", "VR_RANK_MAX", "VR_FILTER_CLAMP", "VR_FILTER_CONSTANT")]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vr.h"\nint main(){' +
                   "".join(f'printf("%zu ", {a});' for a in args) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    D, R = capi.RankDesc, capi.RankResult
    want = [C.sizeof(D)] + [getattr(D, f).offset for f in fields_d] + [C.sizeof(R)] + [getattr(R, f).offset for f in fields_r]
    want += [100 + c for c in (capi.RANK_MAX_RADIUS, capi.RANK_MIN, capi.RANK_MEDIAN, capi.RANK_MAX, capi.FILTER_CLAMP, capi.FILTER_CONSTANT)]
    assert out == want
    assert (C.sizeof(D), C.sizeof(R)) == (64, 32)
    assert (rr.MAX_RADIUS, rr.MIN, rr.MEDIAN, rr.MAX) == (capi.RANK_MAX_RADIUS, capi.RANK_MIN, capi.RANK_MEDIAN, capi.RANK_MAX) == (3, 0, -1, -2)
    assert (rr.CLAMP, rr.CONSTANT) == (capi.FILTER_CLAMP, capi.FILTER_CONSTANT)


def test_entry_points_without_a_device():
    """Every entry point refuses a NULL context (or a NULL output) with VR_ERR_INVALID_ARG; the symbols are exported."""
    lib = capi.load()
    d = capi.RankDesc()
    assert lib.vr_rank_whole(None, 0, 3, 1, 3, C.byref(d)) == capi.VR_ERR_INVALID_ARG
    assert lib.vr_volume_rank(None, C.byref(d), None) == capi.VR_ERR_INVALID_ARG
    assert lib.vr_rank_counters(None, None) == capi.VR_ERR_INVALID_ARG and lib.vr_rank_timing(None, None) == capi.VR_ERR_INVALID_ARG
    for name in ("vr_rank_whole", "vr_volume_rank", "vr_rank_counters", "vr_rank_timing"):
        assert name in capi.ABI_SYMBOLS and hasattr(lib, name)
    from volumerendering_amd import host
    assert hasattr(host.load(), "vrh_app_rank")


def test_rank_desc_copy_and_result_tuple():
    d = capi.RankDesc()
    e = d.copy(src_slot=2, src_channel=1, dst_slot=1, dst_channel=3, radius=(1, 2, 3), rank=capi.RANK_MAX, border=1, border_value=-2.5,
               box_lo=(1, 2, 3), box_hi=(4, 5, 6))
    assert (e.src_slot, e.src_channel, e.dst_slot, e.dst_channel, list(e.radius), e.rank, e.border, e.border_value) == (2, 1, 1, 3, [1, 2, 3], -2, 1, -2.5)
    assert list(e.box_lo) == [1, 2, 3] and list(e.box_hi) == [4, 5, 6]
    assert d.border == 0 and d.rank == 0 and bytes(e.copy()) == bytes(e)
    r = capi.RankResult(5, 1, 3, -0.0, 2.0)
    assert r.as_tuple() == (5, 1, 3, 0x80000000, 0x40000000)


# ---- the restatement -------------------------------------------------------------------------------------------------------------------

def bits(a):
    return np.ascontiguousarray(a, f32).view(u32)


@pytest.fixture(scope="module")
def field():
    """Finite data without -0.0, a fifth of the voxels one repeated value, and +-inf."""
    rng = np.random.default_rng(7)
    v = rng.normal(0.0, 1.0, (9, 12, 40)).astype(f32)
    v[v == 0] = f32(1.0)
    v[rng.random(v.shape) < 0.2] = f32(0.375)
    v[rng.random(v.shape) < 0.02] = f32(np.inf)
    v[rng.random(v.shape) < 0.02] = f32(-np.inf)
    return v


RADII = {1: (0, 0, 0), 15: (1, 2, 0), 21: (1, 3, 0), 27: (1, 1, 1), 105: (1, 2, 3), 125: (2, 2, 2), 343: (3, 3, 3)}  # (x, y, z) by window


@pytest.mark.parametrize("border", [rr.CLAMP, rr.CONSTANT], ids=["clamp", "constant"])
@pytest.mark.parametrize("n", sorted(RADII))
def test_restatement_is_scipys_rank_filter(field, n, border):
    """Bit-equal to scipy.ndimage.rank_filter at ranks 0, N / 3, N / 2 and N - 1, and to median_filter, minimum_filter and maximum_filter,
    with both borders and a nonzero cval."""
    ndi = pytest.importorskip("scipy.ndimage")
    radii = RADII[n]
    assert rr.window(radii) == n
    size = tuple(2 * r + 1 for r in radii[::-1])
    kw = dict(size=size, mode=MODE[border], cval=-1.5)
    for k in sorted({0, n // 3, n // 2, n - 1}):
        got = rr.select(field, radii, k, border, rr.bits_of(-1.5))
        assert np.array_equal(got, bits(ndi.rank_filter(field, rank=k, **kw))), (n, k)
    assert np.array_equal(rr.select(field, radii, rr.MEDIAN, border, rr.bits_of(-1.5)), bits(ndi.median_filter(field, **kw)))
    assert np.array_equal(rr.select(field, radii, rr.MIN, border, rr.bits_of(-1.5)), bits(ndi.minimum_filter(field, **kw)))
    assert np.array_equal(rr.select(field, radii, rr.MAX, border, rr.bits_of(-1.5)), bits(ndi.maximum_filter(field, **kw)))


def test_box_channels_counters_and_result_of_the_restatement():
    """By hand on one row: the box limits what is stored, not what is read; the borders; the untouched bits; changed; the counters; the
    total order over -0.0f, +0.0f and NaNs of both signs; payloads survive."""
    src = np.zeros((1, 1, 6, 4), f32)
    src[0, 0, :, 3] = [1, 9, 4, 8, 2, 32]
    before = np.full((1, 1, 6, 4), 7.0, f32)
    out, res, cnt = rr.rank(src, before, 3, 1, (1, 0, 0), rr.MEDIAN, rr.CLAMP, 0, (1, 0, 0), (6, 1, 1))
    assert out[0, 0, :, 1].tolist() == [7, 4, 8, 4, 8, 32] and (np.delete(out, 1, axis=3) == 7).all()
    assert res == (5, 0, 4, int(bits(f32(4))[0]), int(bits(f32(32))[0])) and cnt == (5, 6, 1)
    out, res, cnt = rr.rank(src, before, 3, 1, (1, 0, 0), rr.MAX, rr.CONSTANT, rr.bits_of(100.0))
    assert out[0, 0, :, 1].tolist() == [100, 9, 9, 8, 32, 100] and res[2] == 4 and cnt == (6, 6, 2)
    out, _, _ = rr.rank(src, before, 3, 1, (1, 0, 0), rr.MIN, rr.CONSTANT, rr.bits_of(-1.0))
    assert out[0, 0, :, 1].tolist() == [-1, 1, 4, 2, 2, -1]
    pats = [0x7FC12345, 0x80000000, 0xFFC00001, 0x00000000, 0xFF800000, 0x7F800001, 0x7F800000, 0x00000001, 0x80000001]
    order = [0xFFC00001, 0xFF800000, 0x80000001, 0x80000000, 0x00000000, 0x00000001, 0x7F800000, 0x7F800001, 0x7FC12345]
    z3 = np.zeros((1, 1, 7, 4), f32)  # (the window of radius 3 around voxel 3 of a row of 7 holds every voxel once)
    z3.view(u32)[0, 0, :, 0] = pats[:7]
    got = [int(bits(rr.rank(z3, None, 0, 2, (3, 0, 0), k, rr.CONSTANT, pats[7], (3, 0, 0), (4, 1, 1))[0])[0, 0, 3, 2]) for k in range(7)]
    assert got == [p for p in order if p in pats[:7]]
    out, res, cnt = rr.rank(z3, None, 0, 2, (0, 0, 0))
    assert res == (7, 5, 0, 0x80000000, 0) and cnt == (7, 7, 0) and bits(out)[0, 0, :, 2].tolist() == pats[:7]
    assert rr.rank(z3, None, 0, 2, (1, 1, 1), lo=(1, 0, 0), hi=(1, 1, 1))[1:] == ((0, 0, 0, 0, 0), (0, 0, 0))
    assert [rr.resolve(k, (1, 1, 1)) for k in (0, 26, 27, -1, -2, -3)] == [0, 26, None, 13, 26, None]
