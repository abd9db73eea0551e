"""CPU side of the lit shader's shadows (vr_set_shadows, include/vr.h): the float32 restatement in shadow_ref.py reproduces the
oracle's LIGHT frames bit for bit when the light volume is 1 everywhere (what an opacity scale of 0 builds); its light-volume build
agrees with float64 in a medium of uniform opacity and leaves T exactly 1 on the light's side of an occluding slab; the library
declares and exports the two entry points without a new variant, and carries both arithmetic modes' shadow kernels, without scratch."""
import os
import re
import sys

import numpy as np
import pytest

import host_ref as hr
import oracle_binding as ob
import shadow_ref as sr
import vrtest as vt
from volumerendering_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import check_exec_regions as cer  # noqa: E402
from march_units import march_units  # noqa: E402

f32 = np.float32
W, H = 40, 32


def uniforms(n, **over):
    step, count = hr.stepping_params(n, n, n)
    kw = dict(steps_count=count, step_size=step)
    kw.update(over)
    return hr.make_uniforms(W, H, **kw)


CAMERAS = [
    # (id, volume kind, uniform overrides)
    ("phantom", "phantom", {}),
    ("side", "phantom", dict(yaw=2.1, pitch=-0.4, distance=1.5)),
    ("clip", "phantom", dict(clip_x=(0.1, 0.2), clip_y=(0.05, 0.0), clip_z=(0.0, 0.3))),
    ("varstep", "sphere", dict(toggles=(1, 0, 0, 0), yaw=-0.8)),
    ("jitter", "phantom", dict(toggles=(0, 1, 0, 0), pitch=0.9)),
    ("jitter_varstep", "sphere", dict(toggles=(1, 1, 0, 0), yaw=1.3, pitch=-0.2)),
]


@pytest.mark.parametrize("cid,kind,over", CAMERAS, ids=[c[0] for c in CAMERAS])
def test_unshadowed_restatement_is_light(cid, kind, over):
    """S = 1 (a light volume of ones, as an opacity scale of 0 builds it, and no light volume at all): the restated march equals the
    oracle's LIGHT frame and composited count bit for bit."""
    v = vt.make_volume(kind, 16, gradient=True)
    tf = (hr.default_opacity_tf(64), hr.default_color_tf(64))
    u = uniforms(16, **over)
    ob.set_arithmetic(ob.SEPARATE)
    ref, n_ref, _ = ob.render(ob.LIGHT, u, [v], [tf], W, H, nthreads=4)
    ones = np.ones((8, 8, 8), f32)
    for grid in (None, ones):
        got, n, cov = sr.frame(u, W, H, v, tf, grid)
        assert n == n_ref > 0
        assert cov > 0
        assert np.array_equal(vt.bits(got), vt.bits(ref)), cid


def test_scale_zero_builds_ones():
    v = vt.make_volume("phantom", 16, gradient=True)
    lo, hi = sr.clip_box(uniforms(16))
    T = sr.build(v, hr.default_opacity_tf(64), 2, 0.0, (0.0, 5.0, 0.0), lo, hi)
    assert T.shape == (8, 8, 8) and np.all(T == f32(1.0))


@pytest.mark.parametrize("a", [0.05, 0.2])
def test_uniform_medium_against_float64(a):
    """Constant density, a constant opacity table of value a, a light far along +y: texel (i, j, k) takes 15 - j steps inside the unit
    cube (half a step of margin on either side), so T = (1 - a)^(15 - j) in float64, within float32's rounding of 15 products."""
    n = 16
    v = np.zeros((n, n, n, 4), f32)
    v[..., 3] = f32(0.5)
    opacity = np.full(64, f32(a))
    lo, hi = sr.clip_box(uniforms(n))
    T = sr.build(v, opacity, 1, 1.0, (0.0, 1.0e4, 0.0), lo, hi)
    j = np.arange(n)[None, :, None]
    expect = np.broadcast_to((1.0 - float(f32(a))) ** (15 - j), T.shape)
    assert np.allclose(T.astype(np.float64), expect, rtol=4e-6, atol=0.0)


@pytest.mark.parametrize("divisor", [1, 2])
def test_slab_occluder(divisor):
    """An opaque slab across y (voxels 6..9) in transparent air, the light above it (+y): every texel whose walk starts two voxels or more
    above the slab keeps T = 1 exactly; every texel below it is in full shadow (T below 2^-10)."""
    n = 16
    v = np.zeros((n, n, n, 4), f32)
    v[:, 6:10, :, 3] = f32(1.0)
    opacity = np.concatenate([np.zeros(32, f32), np.ones(32, f32)])
    lo, hi = sr.clip_box(uniforms(n))
    T = sr.build(v, opacity, divisor, 1.0, (0.0, 5.0, 0.0), lo, hi)
    gy = T.shape[1]
    cy = (np.arange(gy) + 0.5) / gy * n - 0.5  # texel centres in voxel coordinates
    above, below = cy >= 11.0, cy <= 4.0
    assert above.any() and below.any()
    assert np.all(T[:, above, :] == f32(1.0))
    assert np.all(T[:, below, :] < f32(2.0 ** -10))


def test_abi_symbols_without_a_new_variant():
    """vr_set_shadows and vr_shadow_volume are declared, listed and exported; shadows are a setting of LIGHT, not a variant."""
    lib = capi.load()
    header = open(os.path.join(ROOT, "include", "vr.h")).read()
    for name in ("vr_set_shadows", "vr_shadow_volume"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in capi.ABI_SYMBOLS
        assert hasattr(lib, name)
    assert int(re.search(r"VR_VARIANT_COUNT\s*=\s*(\d+)", header).group(1)) == 12
    assert len(capi.VARIANT_NAMES) == 12
    assert callable(getattr(capi.Context, "set_shadows", None)) and callable(getattr(capi.Context, "shadow_volume", None))


@pytest.mark.skipif(not os.path.exists(cer.OBJDUMP), reason="llvm-objdump of the ROCm toolchain not found")
def test_shadow_kernels_in_both_units_without_scratch():
    """Exactly two code objects, the march units of namespace vr and of namespace vrf (march_units), carry shadow kernels: each the 8
    march_shadow_kernel instances (skipping or not, 32- or 64-bit offsets, one frame or several) and the 4 shadow_build_kernel
    instances, and no instruction of theirs touches scratch."""
    for names, scratch, _ in march_units("march_shadow_kernel", "shadow_build_kernel"):
        march = {n for n in names if "march_shadow_kernel" in n}
        assert len(march) == 8, sorted(march)
        assert len(names - march) == 4, sorted(names - march)
        assert not scratch, scratch[:5]
