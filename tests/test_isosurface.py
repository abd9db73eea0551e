"""CPU side of the shaded isosurface (VR_VARIANT_ISO, include/vr.h): the float32 restatement in iso_ref.py reproduces the oracle's
LIGHT frames bit for bit where the two must agree (a level below every sample, a constant colour table and opacity 1: LIGHT blends
its first in-box sample opaquely and stops, which is exactly ISO's fragment); the secant refinement places the surface of an
analytic sphere within a small fraction of a voxel, far closer than the unrefined hit step; and the library exports the entry point
and carries both arithmetic modes' march_iso_kernel instances, without scratch."""
import os
import re
import sys

import numpy as np
import pytest

import host_ref as hr
import iso_ref as ir
import oracle_binding as ob
import vrtest as vt
from volumerendering_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import check_exec_regions as cer  # noqa: E402
from march_units import march_units  # noqa: E402

f32 = np.float32
W, H = 40, 32


def flat_tf(res=64, rgb=(0.8, 0.55, 0.3)):
    """Constant colour, opacity 1 everywhere: LIGHT's first in-box sample is opaque."""
    c = np.tile(np.array([*rgb, 1.0], f32), (res, 1))
    return np.ones(res, f32), c


CASES = [
    # (id, volume kind, uniform overrides)
    ("sphere", "sphere", {}),
    ("phantom", "phantom", {}),
    ("clip", "phantom", dict(clip_x=(0.1, 0.2), clip_y=(0.05, 0.0), clip_z=(0.0, 0.3))),
    ("varstep", "phantom", dict(toggles=(1, 0, 0, 0))),
    ("jitter", "sphere", dict(toggles=(0, 1, 0, 0))),
    ("steps0", "phantom", dict(steps_count=0)),
    ("steps1", "phantom", dict(steps_count=1)),
    ("steps7", "phantom", dict(steps_count=7, step_size=0.05)),
]


def uniforms(n, **over):
    step, count = hr.stepping_params(n, n, n)
    kw = dict(steps_count=count, step_size=step)
    kw.update(over)
    return hr.make_uniforms(W, H, **kw)


@pytest.mark.parametrize("cid,kind,over", CASES, ids=[c[0] for c in CASES])
def test_restatement_reproduces_light_at_the_first_sample(cid, kind, over):
    """iso = -1: every finite sample hits at the ray's first in-box step, nothing is refined, and the ISO restatement equals the
    oracle's LIGHT frame and its composited count (the restatement models the separately rounded mode)."""
    v = vt.make_volume(kind, 16, gradient=True)
    tf = flat_tf()
    u = uniforms(16, **over)
    ob.set_arithmetic(ob.SEPARATE)
    ref, n_ref, _ = ob.render(ob.LIGHT, u, [v], [tf], W, H, nthreads=4)
    got, n, cov = ir.frame(u, W, H, v, tf, -1.0)
    assert n == n_ref
    assert np.array_equal(vt.bits(got), vt.bits(ref))
    if cid not in ("steps0",):
        assert cov > 0


def test_restatement_shades_a_refined_point():
    """A level between voxel values: most hits are refined (q differs from p_k), the fragment is opaque with the level's colour
    scaled by the light, and no-hit pixels are exactly zero."""
    v = vt.make_volume("phantom", 16, gradient=True)
    tf = (hr.default_opacity_tf(64), hr.default_color_tf(64))
    u = uniforms(16)
    r = ir.march(u, W, H, v, tf, 0.3)
    hit = r["hit"]
    assert hit.sum() > 50
    assert np.all(r["frag"][hit, 3] == f32(1.0)) and not np.any(r["frag"][~hit])
    moved = np.any(r["q"][hit] != r["pk"][hit], axis=1)
    assert moved.mean() > 0.8


def sphere_distance_volume(n=32, radius=10.0, slope=0.02):
    """density = 0.5 + slope * (radius - r), r = distance in voxels from the volume's centre: the level 0.5 is a sphere of `radius`
    voxels (texel centres at (i + 0.5) / n)."""
    i = np.arange(n, dtype=np.float64) - (n - 1) / 2.0
    z, y, x = np.meshgrid(i, i, i, indexing="ij")
    r = np.sqrt(x * x + y * y + z * z)
    v = np.zeros((n, n, n, 4), f32)
    v[..., 3] = (0.5 + slope * (radius - r)).astype(f32)
    return v


def test_refinement_against_float64_surface():
    """On an analytic sphere-distance volume the refined hit points lie within 0.05 voxel of the float64 surface (trilinear
    filtering of the distance field and the secant's chord are the only errors), and their mean error is far below that of the
    unrefined hit steps p_k (about half a step)."""
    n, R = 32, 10.0
    v = sphere_distance_volume(n, R)
    tf = (hr.default_opacity_tf(64), hr.default_color_tf(64))
    u = uniforms(n, distance=1.4, yaw=0.4, pitch=0.3)
    r = ir.march(u, W, H, v, tf, 0.5)
    hit = r["hit"]
    assert hit.sum() > 60

    def err(pts):
        vox = pts.astype(np.float64) * n - 0.5 - (n - 1) / 2.0
        return np.abs(np.linalg.norm(vox, axis=1) - R)

    e_q, e_p = err(r["q"][hit]), err(r["pk"][hit])
    assert e_q.max() < 0.05, e_q.max()
    assert e_q.mean() < 0.1 * e_p.mean(), (e_q.mean(), e_p.mean())


def test_abi_symbol_and_constant():
    lib = capi.load()
    assert hasattr(lib, "vr_set_iso_value") and "vr_set_iso_value" in capi.ABI_SYMBOLS
    header = open(os.path.join(ROOT, "include", "vr.h")).read()
    assert int(re.search(r"VR_VARIANT_ISO\s*=\s*(\d+)", header).group(1)) == capi.ISO == 11
    assert int(re.search(r"VR_VARIANT_COUNT\s*=\s*(\d+)", header).group(1)) == 12
    assert capi.VARIANT_NAMES[capi.ISO] == "ISO"


@pytest.mark.skipif(not os.path.exists(cer.OBJDUMP), reason="llvm-objdump of the ROCm toolchain not found")
def test_iso_kernels_in_both_units_without_scratch():
    """Exactly two code objects, the march units of namespace vr (separate multiply-adds) and of namespace vrf (fused; march_units),
    carry the 8 march_iso_kernel instances each -- skipping or not, 32- or 64-bit offsets, one frame or several -- and no instruction
    of theirs touches scratch."""
    for names, scratch, _ in march_units("march_iso_kernel"):
        assert len(names) == 8, sorted(names)
        assert not scratch, scratch[:5]
