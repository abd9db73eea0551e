"""CPU side of the slice views (vr_slice_async, include/vr.h; csrc/vr_slice.h): the float32 restatement in slice_ref.py returns the
voxels themselves on voxel-centre planes, agrees with a float64 evaluation of the same positions within a bound counted from its
operations, and the brick record the kernel reads for a NEAREST sample bounds the voxel it addresses; the ABI and the code objects
carry what the header promises."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import slice_ref as sr
import wgsl_f64 as wf
from volumerendering_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import check_exec_regions as cer  # noqa: E402
from march_units import march_units, once_in_the_abi_unit  # noqa: E402

f32 = np.float32


def noise_volume(shape, seed=5):
    """vec4 voxels [nz, ny, nx, 4] with .a in [0, 1) (multiples of 2^-12: every voxel a distinct-looking, exact f32)."""
    nx, ny, nz = shape
    a = np.random.default_rng(seed).integers(0, 4096, size=(nz, ny, nx)).astype(f32) / f32(4096.0)
    v = np.zeros((nz, ny, nx, 4), f32)
    v[..., 3] = a
    return v


@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("filt", [sr.LINEAR, sr.NEAREST])
@pytest.mark.parametrize("reduce", [sr.MAX, sr.MIN, sr.AVERAGE])
@pytest.mark.parametrize("fused", [False, True])
def test_voxel_centre_planes_return_the_voxels(axis, filt, reduce, fused):
    """16^3, the orthogonal descriptor, thickness 1: (i + 0.5) / 16 and every product with 16 are exact, every lerp fraction is 0,
    a + (b - a) * 0 = a -- so the reduced value of each pixel is the voxel's .a bit for bit, whatever the sampler restates."""
    v = noise_volume((16, 16, 16))
    for index in (0, 7, 15):
        d = sr.orthogonal_desc((16, 16, 16), axis, index, 1).copy(reduce=reduce, filter=filt)
        val, n, _ = sr.reduce_slab(d, v, fused=fused)
        ua, va = (1 if axis == 0 else 0), (1 if axis == 2 else 2)
        assert (d.width, d.height) == (16, 16) and np.all(n == 1)
        idx = [slice(None)] * 3
        idx[axis] = index
        plane = v[..., 3][idx[2], idx[1], idx[0]]  # [the later axis, the earlier axis] = [py, px]
        assert ua < va
        assert np.array_equal(val.reshape(16, 16).view(np.uint32), np.ascontiguousarray(plane).view(np.uint32))


def oblique_desc(shape, W=40, H=24, steps=7, **over):
    """A plane tilted against all three axes that leaves the cube in one corner (pixels with n == 0)."""
    d = capi.SliceDesc()
    d.volume_slot, d.tf_slot, d.width, d.height, d.slab_steps = 0, 0, W, H, steps
    d = d.copy(origin=(0.07, -0.05, 0.31), du=(0.9 / W, 0.35 / W, 0.2 / W), dv=(-0.2 / H, 1.0 / H, 0.45 / H), dn=(0.011, -0.013, 0.023))
    return d.copy(**over)


@pytest.mark.parametrize("reduce", [sr.MAX, sr.MIN, sr.AVERAGE])
def test_reductions_match_float64(reduce):
    """The three reductions on a 24 x 20 x 12 volume and an oblique 33-step slab against a float64 evaluation of the SAME positions
    (the f32 positions, converted exactly) with wgsl_f64's sampler.  The bound, from the f32 operations, with u = 2^-24, voxels in
    [0, 1) (M = 1, neighbouring voxels differ by at most L = 1) and N = 24 the largest axis:
      texture coordinate p * N - 0.5: the product errs by at most N u (the subtraction of 0.5 is exact above 0.25, and below it
        the pair is clamped to one texel), which moves the continuous trilinear function by at most L N u per axis: 3 N L u;
      seven lerps, three levels deep, three roundings each on magnitudes <= M: 3 u M per lerp, and a lerp passes its inputs'
        errors on with weights (1 - t, t): 9 u M per sample;
      MAX / MIN of perturbed samples move by no more than the largest perturbation;
      AVERAGE: n - 1 rounded additions of partial sums <= n M, then one division: the mean errs by at most (n - 1) u M + u M.
    So tol = (3 N L + 9 M + n M) u with n = 33 steps."""
    shape = (24, 20, 12)
    v = noise_volume(shape, seed=9)
    d = oblique_desc(shape, steps=33, reduce=reduce)
    val, n, pix = sr.reduce_slab(d, v)
    u = 2.0 ** -24
    tol = (3 * 24 * 1.0 + 9 * 1.0 + 33 * 1.0) * u
    vol = wf.Volume(v)
    p = sr.positions(d, pix)
    dn = np.array(list(d.dn), f32)
    acc = [[] for _ in range(len(pix))]
    for _ in range(33):
        inb = sr.in_cube(p)
        vals = vol.linear(p.astype(np.float64))[:, 3]
        for k in np.nonzero(inb)[0]:
            acc[k].append(vals[k])
        p = p + dn[None, :]
    assert 0 < int((n == 0).sum()) < len(pix) and int(n.max()) > 20
    for k in np.nonzero(n)[0]:
        assert len(acc[k]) == n[k]
        ref = max(acc[k]) if reduce == sr.MAX else (min(acc[k]) if reduce == sr.MIN else float(np.mean(acc[k])))
        assert abs(float(val[k]) - ref) <= tol, (k, float(val[k]), ref, tol)


@pytest.mark.parametrize("fused", [False, True])
def test_base_cell_brick_bounds_the_nearest_voxel(fused):
    """Adversarial search for a counted position whose NEAREST voxel lies outside the footprint of the brick the kernel reads the
    record of (csrc/vr_slice.h: brick b of the base cell covers the voxels 4 b .. min(4 b + 4, n - 1)): grid sizes 1 .. 65535,
    positions on and next to k / n and (k + 0.5) / n, where either floor can tip, and the faces."""
    rng = np.random.default_rng(17)
    N = 300_000
    bad = 0
    for trial in range(4):
        n = rng.integers(1, 65536, size=N) if trial < 2 else rng.choice([1, 2, 3, 4, 5, 7, 12, 16, 20, 24, 255, 512, 1023], size=N)
        nf = n.astype(f32)
        k = np.floor(rng.random(N) * (n + 1)).astype(np.int64)
        half = np.where(rng.random(N) < 0.5, 0.5, 0.0)
        p = ((k + half) / n).astype(f32)
        for _ in range(3):  # a few ulps to either side
            step = rng.integers(-3, 4, size=N)
            p = np.where(step > 0, np.nextafter(p, f32(2)), np.where(step < 0, np.nextafter(p, f32(-1)), p)).astype(f32)
        if trial == 1:
            p = rng.random(N).astype(f32)
        p = np.clip(p, f32(0), f32(1))  # counted positions only
        i = np.clip(np.floor(p * nf).astype(np.int64), 0, n - 1)
        bn = (n + 3) >> 2
        bs = nf * f32(0.25)
        x = sr.fma32(p, bs, f32(-0.125)) if fused else (p * bs + f32(-0.125)).astype(f32)
        b = np.clip(x, f32(0), (bn - 1).astype(f32)).astype(np.int64)  # (v_med3_f32, then truncation)
        bad += int(np.sum((i < 4 * b) | (i > np.minimum(4 * b + 4, n - 1))))
    assert bad == 0


def test_abi_symbols_struct_and_null_context():
    lib = capi.load()
    header = open(os.path.join(ROOT, "include", "vr.h")).read()
    for name in ("vr_slice_async", "vr_slice_render", "vr_slice_orthogonal", "vr_slice_counters"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in capi.ABI_SYMBOLS
        assert hasattr(lib, name)
    # struct vr_slice_desc: 4 x 4 + 4 x 12 + 4 x 4 bytes, no padding; the enumerators as the header defines them
    assert C.sizeof(capi.SliceDesc) == 80
    body = re.search(r"typedef struct vr_slice_desc \{(.*?)\} vr_slice_desc;", header, re.S).group(1)
    fields = re.findall(r"\b(?:int32_t|uint32_t|float)\s+([^;]+);", body)
    names = [re.sub(r"\[\d+\]", "", f.strip()) for decl in fields for f in decl.split(",")]
    assert names == [f[0] for f in capi.SliceDesc._fields_]
    for macro, value in (("VR_SLICE_MAX", capi.SLICE_MAX), ("VR_SLICE_MIN", capi.SLICE_MIN), ("VR_SLICE_AVERAGE", capi.SLICE_AVERAGE),
                         ("VR_SLICE_LINEAR", capi.SLICE_LINEAR), ("VR_SLICE_NEAREST", capi.SLICE_NEAREST),
                         ("VR_SLICE_RGBA32F", capi.SLICE_RGBA32F), ("VR_SLICE_BGRA8", capi.SLICE_BGRA8)):
        assert int(re.search(r"#define\s+" + macro + r"\s+(\d+)", header).group(1)) == value
    assert int(re.search(r"VR_VARIANT_COUNT\s*=\s*(\d+)", header).group(1)) == 12 and len(capi.VARIANT_NAMES) == 12
    assert int(re.search(r"#define\s+VR_ABI_VERSION\s+(\d+)", header).group(1)) == 1
    for m in ("slice_async", "slice", "slice_orthogonal", "slice_counters"):
        assert callable(getattr(capi.Context, m, None)), m
    d, out = capi.SliceDesc(), (C.c_uint64 * 3)()
    assert lib.vr_slice_async(None, C.byref(d), None, None) == capi.VR_ERR_INVALID_ARG
    assert lib.vr_slice_render(None, C.byref(d), None) == capi.VR_ERR_INVALID_ARG
    assert lib.vr_slice_orthogonal(None, 0, 0, 0, 1, C.byref(d)) == capi.VR_ERR_INVALID_ARG
    assert lib.vr_slice_counters(None, C.byref(out)) == capi.VR_ERR_INVALID_ARG


@pytest.mark.skipif(not os.path.exists(cer.OBJDUMP), reason="llvm-objdump of the ROCm toolchain not found")
def test_slice_kernels_in_both_units_without_scratch():
    """Exactly two code objects, the march units of namespace vr and of namespace vrf (march_units), carry the 24 slice_kernel
    instances each -- three reductions x two filters x 32- / 64-bit offsets x skipping or not -- and no instruction of theirs touches
    scratch.  slice_sum_kernel exists once, in the C ABI's unit, without scratch."""
    for names, scratch, _ in march_units("slice_kernel"):
        assert len(names) == 24, sorted(names)
        assert not scratch, scratch[:5]
    assert not once_in_the_abi_unit("slice_sum_kernel")[1]


def test_bench_tool_help():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "slice_bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "slice" in r.stdout.lower()
