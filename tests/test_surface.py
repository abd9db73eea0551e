"""CPU side of the surface-position output (vr_set_output, include/vr.h, csrc/vr_surf.h): the float32 restatement in surf_ref.py is
pinned to the oracle -- at tau = 0.95f its .w plane and composited count are the oracle's BASIC alpha plane and count bit for bit, at
tau = 0x1.fffffep-1f LIGHT's --, its hits obey the properties the definition implies (q between p_{k-1} and p_k, monotone in tau,
hit <=> .w > tau), the isosurface's surface output is iso_ref's refined point, and the library declares, lists and exports the entry
points, validates the threshold and carries both arithmetic modes' march_surf_kernel instances, without scratch."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import host_ref as hr
import iso_ref as ir
import oracle_binding as ob
import surf_ref as sr
import vrtest as vt
from volumerendering_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import check_exec_regions as cer  # noqa: E402
from march_units import march_units, once_in_the_abi_unit  # noqa: E402

f32 = np.float32
W, H = 40, 32


def steep_tf(res=64, gain=4.0):
    """Opacity min(1, gain * ramp) (exactly 0 at density 0) under the default colour ramp: rays through tissue pass 0.95 and reach
    1.0 within a few steps, which the default ramp on a 16^3 volume does not for every case below."""
    o = np.minimum(hr.default_opacity_tf(res) * f32(gain), f32(1.0)).astype(f32)
    return o, hr.default_color_tf(res)


# the case list of test_isosurface.py; `hits`: the case is meant to have some (checked against the ORACLE's alpha plane below)
CASES = [
    ("sphere", "sphere", {}, True),
    ("phantom", "phantom", {}, True),
    ("clip", "phantom", dict(clip_x=(0.1, 0.2), clip_y=(0.05, 0.0), clip_z=(0.0, 0.3)), True),
    ("varstep", "phantom", dict(toggles=(1, 0, 0, 0)), True),
    ("jitter", "sphere", dict(toggles=(0, 1, 0, 0)), True),
    ("steps0", "phantom", dict(steps_count=0), False),
    ("steps1", "phantom", dict(steps_count=1), False),
    ("steps7", "phantom", dict(steps_count=7, step_size=0.05), True),
]


def uniforms(n, **over):
    step, count = hr.stepping_params(n, n, n)
    kw = dict(steps_count=count, step_size=step)
    kw.update(over)
    return hr.make_uniforms(W, H, **kw)


@pytest.mark.parametrize("variant,tau", [(ob.BASIC, sr.TAU_BASIC), (ob.LIGHT, sr.TAU_LIGHT)], ids=["basic", "light"])
@pytest.mark.parametrize("cid,kind,over,hits", CASES, ids=[c[0] for c in CASES])
def test_alpha_plane_and_count_are_the_oracles(cid, kind, over, hits, variant, tau):
    """At the shader's own cut-off the surface march blends exactly the samples the shader blends: .w is the oracle's alpha plane and
    the composited count the oracle's, bit for bit (the restatement models the separately rounded mode)."""
    v = vt.make_volume(kind, 16, gradient=True)
    tf = steep_tf()
    u = uniforms(16, **over)
    ob.set_arithmetic(ob.SEPARATE)
    ref, n_ref, _ = ob.render(variant, u, [v], [tf], W, H, nthreads=4)
    got, n, cov = sr.frame(u, W, H, v, tf[0], tau)
    print(cid, "oracle alpha max", float(ref[..., 3].max()), "hits", cov, "composited", n)
    assert n == n_ref
    assert np.array_equal(vt.bits(got[..., 3]), vt.bits(ref[..., 3]))
    assert cov == int((ref[..., 3] > tau).sum())
    if hits:
        assert cov > 0


@pytest.mark.parametrize("cid,kind,over,hits", CASES, ids=[c[0] for c in CASES])
def test_hit_properties(cid, kind, over, hits):
    """Properties that need no measured number: a hit's q lies component-wise between p_{k-1} and p_k (it is p_k on the ray's first
    in-box step); hit <=> .w > tau; pixels without a hit have zero xyz; for tau1 < tau2 the hit step does not come earlier and, on the
    same step, q does not move back along the ray."""
    v = vt.make_volume(kind, 16, gradient=True)
    o = steep_tf()[0]
    u = uniforms(16, **over)
    runs = {tau: sr.march(u, W, H, v, o, tau) for tau in (0.0, 0.25, 0.5, 0.95)}
    for tau, r in runs.items():
        hit = r["hit"]
        assert np.array_equal(hit, r["frag"][:, 3] > f32(tau))
        assert not np.any(r["frag"][~hit, :3])
        assert not np.any(r["frag"][~r["rayhit"]])
        first = hit & r["first"]
        assert np.array_equal(vt.bits(r["q"][first]), vt.bits(r["pk"][first]))
        mid = hit & ~r["first"]
        lo, hi = np.minimum(r["pp"][mid], r["pk"][mid]), np.maximum(r["pp"][mid], r["pk"][mid])
        assert np.all((r["q"][mid] >= lo) & (r["q"][mid] <= hi))
        assert np.array_equal(vt.bits(r["frag"][hit, :3]), vt.bits(r["q"][hit]))
    if hits:
        assert runs[0.5]["hit"].sum() > 0
    taus = sorted(runs)
    for t1, t2 in zip(taus, taus[1:]):
        a, b = runs[t1], runs[t2]
        both = a["hit"] & b["hit"]
        assert not np.any(b["hit"] & ~a["hit"])  # a hit at the higher threshold is one at the lower
        assert np.all(b["k"][both] >= a["k"][both])
        same = both & (a["k"] == b["k"]) & ~a["first"]
        # along the ray: (q2 - q1) . (p_k - p_{k-1}) >= 0 per component (the step's sign)
        d = (b["q"][same].astype(np.float64) - a["q"][same]) * np.sign(a["pk"][same].astype(np.float64) - a["pp"][same])
        assert np.all(d >= 0.0)


def test_iso_surface_is_the_refined_point():
    v = vt.make_volume("phantom", 16, gradient=True)
    tf = (hr.default_opacity_tf(64), hr.default_color_tf(64))
    u = uniforms(16)
    r = ir.march(u, W, H, v, tf, 0.3)
    frag, n, cov = sr.iso_frame(u, W, H, v, tf, 0.3)
    hit = r["hit"]
    assert hit.sum() > 50 and cov == hit.sum() and n == r["composited"].sum()
    flat = frag.reshape(-1, 4)
    assert np.array_equal(vt.bits(flat[hit, :3]), vt.bits(r["q"][hit]))
    assert np.all(flat[hit, 3] == f32(1.0)) and not np.any(flat[~hit])


def test_depth_and_pick_record():
    """The depth of a hit lies inside (0, 1), equals a float64 evaluation of the same matrices to rounding and grows along the view axis; pixels without a hit are at 1.0; the pick
    record's voxel is the one that contains the point and its value the uploaded voxel."""
    v = vt.make_volume("phantom", 16, gradient=True)
    tf = steep_tf()
    u = uniforms(16)
    frag, _, cov = sr.frame(u, W, H, v, tf[0], 0.5)
    assert cov > 50
    d = sr.depth(frag, u, 0.5)
    hit = frag[..., 3] > f32(0.5)
    assert np.all(d[~hit] == f32(1.0)) and np.all((d[hit] > 0.0) & (d[hit] < 1.0))
    # an independent float64 evaluation of proj * view * (world, 1).  Bound: about twenty float32 operations on magnitudes below 2,
    # each within 2^-24 relative -> 20 * 6e-8 * 2 = 2.4e-6; 1e-5 asserted.
    view, proj = (np.array(list(m), np.float64).reshape(4, 4).T for m in (u.view, u.proj))
    wpts = np.concatenate([sr.world_of(frag[hit][:, :3]).astype(np.float64), np.ones((hit.sum(), 1))], 1)
    clip = (proj @ view @ wpts.T).T
    assert np.max(np.abs(d[hit] - clip[:, 2] / clip[:, 3])) < 1e-5
    eye_z = (view @ wpts.T).T[:, 2]  # (the camera looks down -z: farther points have the larger depth)
    order = np.argsort(-eye_z)
    assert np.all(np.diff((clip[:, 2] / clip[:, 3])[order]) >= 0.0)
    ys, xs = np.nonzero(hit)
    rec = sr.pick(sr.BASIC, u, W, H, [v, None, None], tf, 0.5, int(xs[0]), int(ys[0]))
    assert rec["hit"] == 1 and np.array_equal(vt.bits(rec["uvw"]), vt.bits(frag[ys[0], xs[0], :3]))
    assert np.all(rec["voxel"] == np.clip(np.floor(rec["uvw"].astype(np.float64) * 16), 0, 15))
    assert np.array_equal(vt.bits(rec["value"][0]), vt.bits(v[rec["voxel"][2], rec["voxel"][1], rec["voxel"][0]]))
    assert not np.any(rec["value"][1:])
    miss = sr.pick(sr.BASIC, u, W, H, [v, None, None], tf, 0.5, 0, 0)
    assert miss["hit"] == 0 and miss["depth"] == f32(1.0) and not np.any(miss["uvw"])


def test_abi_symbols_without_a_new_variant():
    """The four entry points are declared, listed and exported; the output is a setting, not a variant."""
    lib = capi.load()
    header = open(os.path.join(ROOT, "include", "vr.h")).read()
    for name in ("vr_set_output", "vr_set_surface_threshold", "vr_surface_depth_async", "vr_pick"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in capi.ABI_SYMBOLS
        assert hasattr(lib, name)
    declared = set(re.findall(r"\b(vr_[a-z_0-9]+)\s*\(", header)) - {"vr_ctx", "vr_status", "vr_variant", "vr_uniforms"}
    assert declared == set(capi.ABI_SYMBOLS)
    assert int(re.search(r"VR_VARIANT_COUNT\s*=\s*(\d+)", header).group(1)) == 12 and len(capi.VARIANT_NAMES) == 12
    assert int(re.search(r"#define\s+VR_OUTPUT_SURFACE\s+(\d+)", header).group(1)) == capi.OUTPUT_SURFACE == 1
    for m in ("set_output", "set_surface_threshold", "surface_depth", "pick"):
        assert callable(getattr(capi.Context, m, None)), m
    # struct vr_pick_result: 4 + 12 + 12 + 4 + 4 + 12 + VR_MAX_VOLUMES * 16 bytes, no padding
    assert C.sizeof(capi.PickResult) == 48 + 16 * capi.MAX_VOLUMES
    assert int(re.search(r"#define\s+VR_MAX_VOLUMES\s+(\d+)", header).group(1)) == capi.MAX_VOLUMES


def test_argument_validation_without_a_device():
    """The setters refuse a NULL context before they touch anything (the values themselves are validated on a live context in
    tests/test_surface_gpu.py: a context needs a device)."""
    lib = capi.load()
    assert lib.vr_set_output(None, 1) == capi.VR_ERR_INVALID_ARG
    assert lib.vr_set_surface_threshold(None, C.c_float(0.5)) == capi.VR_ERR_INVALID_ARG
    assert lib.vr_surface_depth_async(None, None, None, None) == capi.VR_ERR_INVALID_ARG
    assert lib.vr_pick(None, 0, 0, 0, None) == capi.VR_ERR_INVALID_ARG


@pytest.mark.skipif(not os.path.exists(cer.OBJDUMP), reason="llvm-objdump of the ROCm toolchain not found")
def test_surf_kernels_in_both_units_without_scratch():
    """Exactly two code objects, the march units of namespace vr (separate multiply-adds) and of namespace vrf (fused; march_units),
    carry surface kernels: each the 8 march_surf_kernel instances -- skipping or not, 32- or 64-bit offsets, one frame or several --
    and the 8 of the isosurface's iso_point_kernel, and no instruction of theirs touches scratch.  surface_depth_kernel exists once,
    in the C ABI's unit, without scratch."""
    for names, scratch, _ in march_units("march_surf_kernel", "iso_point_kernel"):
        surf = {n for n in names if "march_surf_kernel" in n}
        assert len(surf) == 8, sorted(surf)
        assert len(names - surf) == 8, sorted(names - surf)
        assert not scratch, scratch[:5]
    assert not once_in_the_abi_unit("surface_depth_kernel")[1]
