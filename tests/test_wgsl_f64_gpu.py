"""The HIP kernels judged directly against the float64 restatement of the WGSL (tests/wgsl_f64.py), with the comparator
and cases of tests/test_wgsl_f64.py: the default kernel choice, the no-skipping kernel (flavour 1) and every shipped
kernel form, in both arithmetic modes; the device data preparation against the f64 preparation; and a seeded spot
check of the full-size C3 and C4 frames."""
import numpy as np
import pytest

import host_ref as hr
import vrtest as vt
import wgsl_cases as wc
import wgsl_f64 as R
from volumerendering_amd import capi, host, workloads as wl

pytestmark = pytest.mark.gpu

FLAVOURS = (0, 1, 6, 7, 8, 10, 11, 12, 13, 15, 16, 17, 18)  # test_parity_gpu.test_every_variant_every_layout's forms
ARITH = (capi.ARITH_SEPARATE, capi.ARITH_FUSED)


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(wc.W, wc.H)
    yield c
    c.set_kernel_flavour(0)
    c.set_arithmetic(capi.ARITH_SEPARATE)
    c.close()


def judge_gpu(ctx, variant, u, vols, tfs, W, H, ref, what):
    if (ctx.width, ctx.height) != (W, H):
        ctx.resize(W, H)
    frag, _, _ = vt.gpu_render(ctx, variant, u, vols, tfs)
    R.assert_matches(frag, None, ref, what)
    assert abs(ctx.covered_pixels() - int(ref.covered.sum())) <= int(ref.graze.sum()), what


@pytest.mark.parametrize("variant,cid", [(v, c[0]) for v in range(8) for c in wc.cases(v)], ids=wc.case_ids())
def test_kernels_match_f64_reference(ctx, variant, cid):
    u, vols, tfs, W, H = wc.inputs(variant, cid)
    ref = wc.reference(variant, cid)
    try:
        for arith in ARITH:
            ctx.set_arithmetic(arith)
            for fl in FLAVOURS:
                ctx.set_kernel_flavour(fl)
                judge_gpu(ctx, variant, u, vols, tfs, W, H, ref, (cid, arith, fl))
    finally:
        ctx.set_kernel_flavour(0)
        ctx.set_arithmetic(capi.ARITH_SEPARATE)


@pytest.mark.parametrize("mode", [1, 2, 3, 4])
def test_debug_modes_match_f64_reference(ctx, mode):
    vols, tfs = wc.scene(R.LIGHT)
    for cam in wc.CAMERAS.values():
        u = hr.make_uniforms(wc.W, wc.H, fragment_mode=mode, **cam)
        judge_gpu(ctx, R.LIGHT, u, vols, tfs, wc.W, wc.H, R.render(R.LIGHT, u, vols, tfs, wc.W, wc.H), (mode, cam))


U = 2.0 ** -24


@pytest.mark.parametrize("shape", [(16, 16, 16), (7, 20, 13), (33, 2, 65)])
def test_device_prep_matches_f64(ctx, shape):
    """vr_volume_upload_raw, then normalise, then gradient (BasicVolLightApp order), and the gradient-first order
    with the [0, 1] normalisation (VolumeMask / MultiCTRT), each against the f64 preparation within the roundings of
    its f32 steps (see test_wgsl_f64.test_prep_matches_f64)."""
    rng = np.random.default_rng(5)
    raw = rng.integers(0, 4096, size=shape, dtype=np.uint16)
    v64 = hr.raw_to_vec4(raw)
    ctx.volume_upload_raw(0, raw)
    ctx.volume_normalize(0)
    n64 = R.normalize_data(v64)
    got = ctx.volume_download(0, shape).astype(np.float64)
    assert (np.abs(got - n64) <= U * np.abs(n64)).all()
    ctx.volume_precompute_gradient(0)
    g64 = R.precompute_gradient(n64)
    got = ctx.volume_download(0, shape).astype(np.float64)
    assert (np.abs(got - g64) <= 3 * U * np.maximum(np.abs(g64), 1.0)).all()
    ctx.volume_upload_raw(1, raw)
    ctx.volume_precompute_gradient(1, True)
    ctx.volume_normalize(1, int(raw.max()))
    a64 = R.normalize_data(R.precompute_gradient(v64, True), int(raw.max()))
    got = ctx.volume_download(1, shape).astype(np.float64)
    assert (np.abs(got - a64) <= 4 * U * np.abs(a64) + 1.2e-38).all()


@pytest.mark.parametrize("workload", ["C3", "C4"])
def test_full_size_spot_check_against_f64(workload):
    """One GPU frame of the full-size scene; 2 048 seeded pixels re-marched in f64 on the same inputs (the f32 volumes
    are read corner by corner and widened, never copied whole)."""
    n, W, H, vname = wl.WORKLOADS[workload]
    with host.Application(W, H, 0) as app:
        variant, vols = wl.build_scene(app, workload, "default", quiet=True)
        app.OnRender()
        frag, _, _ = app.ReadFrame()
        ub, volumes, tfs = wl.oracle_inputs(app, vols)
        rng = np.random.default_rng(2048)
        pxy = np.stack([rng.integers(0, W, 2048), rng.integers(0, H, 2048)], axis=1)
        ref = R.render(variant, hr.Uniforms.from_buffer_copy(ub), volumes, tfs, W, H, pxy=pxy)
        v = R.judge(frag[pxy[:, 1], pxy[:, 0]], None, ref)
        print(workload, v)
        # 886 steps of 1/512: the linear position-drift bound (0.015 texel at the far end) puts a zero-length gradient
        # or a box face within reach of about a fifth of these rays, beyond FRAGILE_MAX.  Every other rule holds, and
        # the rays left are judged in full.
        assert all("fragile pixels" in p for p in v.problems), (workload, v)
        assert v.fragile <= 0.3 * v.covered and ref.covered.sum() > 500 and np.max(ref.frag[:, 3]) > 0.5, v
