"""The CPU oracle against the independent float64 restatement of the WGSL (tests/wgsl_f64.py), for every shader, on
cameras, clips, step rules, jitter, step counts, an anisotropic volume and three TF resolutions, in both arithmetic
modes, with one comparator (wgsl_f64.judge) whose constants are derived in one place.  A mutation self-test shows
that the comparator rejects deliberately wrong variants of the reference, so these checks would fail on a subtly
wrong oracle -- and, through the bit-exact suite, on a subtly wrong kernel."""
import os

import numpy as np
import pytest

import host_ref as hr
import oracle_binding as ob
import wgsl_cases as wc
import wgsl_f64 as R

NTHREADS = min(len(os.sched_getaffinity(0)), 16)
MODES = {"separate": ob.SEPARATE, "fused": ob.FUSED}


def oracle_frame(variant, u, vols, tfs, W, H, mode=ob.SEPARATE):
    with ob.arithmetic(mode):
        frag, _, _ = ob.render(variant, u, vols, tfs, W, H, nthreads=NTHREADS)
    return frag


def covered_mask(u, W, H):
    """The oracle's fragment coverage, from its ray set-up (a covered pixel may still be black)."""
    return np.array([[ob.setup_ray(u, W, H, x, y)[0] for x in range(W)] for y in range(H)])


@pytest.mark.parametrize("variant,cid", [(v, c[0]) for v in range(8) for c in wc.cases(v)], ids=wc.case_ids())
def test_oracle_matches_f64_reference(variant, cid):
    u, vols, tfs, W, H = wc.inputs(variant, cid)
    ref = wc.reference(variant, cid)
    cov = covered_mask(u, W, H)
    for name, mode in MODES.items():
        R.assert_matches(oracle_frame(variant, u, vols, tfs, W, H, mode), cov, ref, (cid, name))
    if u.steps_count > 1:  # sample 0 lies on the box face, in air
        assert np.nanmax(ref.frag[..., 3]) > 0  # the case draws something


@pytest.mark.parametrize("mode", [1, 2, 3, 4])
@pytest.mark.parametrize("variant", [R.BASIC, R.LIGHT, R.VOLUME_MASK])
def test_debug_modes_match_f64_reference(variant, mode):
    vols, tfs = wc.scene(variant)
    for cam in ("default", "oblique", "close"):
        u = hr.make_uniforms(wc.W, wc.H, fragment_mode=mode, **wc.CAMERAS[cam])
        ref = R.render(variant, u, vols, tfs, wc.W, wc.H)
        frame = oracle_frame(variant, u, vols, tfs, wc.W, wc.H)
        v = R.assert_matches(frame, covered_mask(u, wc.W, wc.H), ref, (mode, cam))
        assert v.fragile == 0 and (frame[ref.covered, 3] == 1).all()


# ---- host data preparation ------------------------------------------------------------------------------------------
U = 2.0 ** -24


def close_f32(a, b, ulps):
    """|a - b| within `ulps` f32 roundings of b (plus the smallest normal for the zeros)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b) <= ulps * U * np.abs(b) + 1.2e-38


@pytest.mark.parametrize("shape", [(16, 16, 16), (7, 20, 13), (1, 3, 2)])
def test_prep_matches_f64(shape):
    raw = hr.ct_phantom_raw(max(shape))[:shape[0], :shape[1], :shape[2]]
    raw = np.ascontiguousarray(raw)
    raw.flat[0] = 4000  # a non-zero maximum for the tiny shapes
    v = hr.raw_to_vec4(raw)
    # normalise, then gradient (BasicVolLightApp order): one division, then a difference of two rounded values
    n32 = ob.normalize_data(v)
    n64 = R.normalize_data(v)
    assert close_f32(n32, n64, 1).all()
    g32 = ob.precompute_gradient(n32)
    g64 = R.precompute_gradient(n64)
    # each f32 input carries 1 rounding; the difference of two such (relative to the larger) adds 1 more
    scale = np.maximum(np.abs(g64), np.abs(n64[..., 3:4]).max())
    assert (np.abs(g32 - g64) <= 3 * U * scale).all()
    # gradient normalised to [0, 1], then normalisation by the raw maximum (VolumeMask / MultiCTRT order): exact
    # differences of integers, one division by the largest length (itself within 2 roundings), one more division
    for norm01 in (True, False):
        a32 = ob.normalize_data(ob.precompute_gradient(v, norm01), int(raw.max()))
        a64 = R.normalize_data(R.precompute_gradient(v, norm01), int(raw.max()))
        assert close_f32(a32, a64, 4).all(), norm01
        if norm01:
            assert abs(np.sqrt((a64[..., :3] ** 2).sum(-1)).max() - 1.0) < 1e-12


# ---- mutation self-test: every deliberately wrong reference is rejected -------------------------------------------
MUTANT_CASES = {
    "vol_half_texel": [(R.BASIC, "cam-default")],
    "tf_half_texel": [(R.BASIC, "aniso-tf16")],
    "late_start": [(R.BASIC, "cam-default")],
    "steps_plus_one": [(R.BASIC, "short-7")],
    "basic_cutoff_swapped": [(R.BASIC, "cam-default")],
    "light_world_step_after_override": [(R.LIGHT, "varstep-jitter")],
    "inshader_gradient_sign": [(R.LIGHT_INSHADER, "cam-default")],
    "mask_r_only": [(R.VOLUME_MASK, "cam-default")],
    "mask_tables_swapped": [(R.VOLUME_MASK, "cam-default")],
    "rt_mix_swapped": [(R.THREE_FILES, "cam-default"), (R.MULTI_CTRT, "cam-default")],
    "ctrt_no_gradient_modulation": [(R.MULTI_CTRT, "cam-default")],
    "ctrt_kd_2_5": [(R.MULTI_CTRT, "cam-default")],
    "illustrative_dist_unclamped": [(R.ILLUSTRATIVE, c) for c in ("cam-default", "cam-oblique", "cam-behind")],
    "illustrative_no_alpha_factor": [(R.ILLUSTRATIVE, "cam-default")],
    "calib_mask_linear": [(R.TF_CALIB, "cam-default")],
}


def test_every_mutant_has_cases():
    assert sorted(MUTANT_CASES) == sorted(R.MUTANTS)


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_mutant_is_rejected(mutant):
    """The oracle frame passes against the reference (test_oracle_matches_f64_reference) and fails against the
    mutant on at least one of the cases listed for it."""
    verdicts = []
    for variant, cid in MUTANT_CASES[mutant]:
        u, vols, tfs, W, H = wc.inputs(variant, cid)
        frame = oracle_frame(variant, u, vols, tfs, W, H)
        assert R.judge(frame, None, wc.reference(variant, cid)).ok
        verdicts.append(R.judge(frame, None, wc.reference(variant, cid, mutant)))
    assert any(not v.ok for v in verdicts), (mutant, verdicts)
