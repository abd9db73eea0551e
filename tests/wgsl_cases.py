"""The scenes that tests/test_wgsl_f64.py (oracle) and tests/test_wgsl_f64_gpu.py (HIP kernels) judge against the
float64 reference tests/wgsl_f64.py, with the reference frames cached per case."""
from __future__ import annotations

import functools
import math

import numpy as np

import host_ref as hr
import oracle_binding as ob
import vrtest as vt
import wgsl_f64 as R

f32 = np.float32
W, H = 48, 40
N = 16

CAMERAS = {
    "default": dict(),
    "oblique": dict(yaw=2.0, pitch=-0.4),
    "close": dict(distance=0.27, yaw=0.0, pitch=0.0),  # just outside the +z face: every ray crosses the whole depth
    "axis": dict(yaw=math.pi / 2, pitch=0.0),
    "behind": dict(yaw=math.pi, pitch=0.2),
}


def stepping(n):
    """MiniApp's recommended count with a step of 1 / (n + 1/2) instead of 1 / n.  With 1 / n a sample lands exactly on
    the far face of an axis-aligned chord of length 1 and ILLUSTRATIVE's distance exactly on its clamp at 1, so the
    outcome is decided by the last bit of the f32 sum, which no reference at another precision can predict."""
    return f32(1.0 / (n + 0.5)), int(math.sqrt(3) * n)


def zero_prefix_tf(res, zeros, top=0.6):
    """Opacity 0 on the first `zeros` texels, then a ramp to `top`; the default grey ramp for colour."""
    o = np.zeros(res, dtype=f32)
    o[zeros:] = np.linspace(0.0, top, res - zeros, dtype=np.float64).astype(f32)
    return o, hr.default_color_tf(res)


def aniso_scene(variant, tf_res, zeros):
    """A 13 x 20 x 7 (nx, ny, nz) window of the phantom, mask and dose; TF tables of resolution tf_res with a zero
    prefix.  Prepared in each scene's own order."""
    def win(a):
        return np.ascontiguousarray(a[6:13, :, 3:16])
    raw = win(hr.ct_phantom_raw(20))
    v = hr.raw_to_vec4(raw)
    if variant in (R.VOLUME_MASK, R.MULTI_CTRT, R.ILLUSTRATIVE):
        ct = ob.normalize_data(ob.precompute_gradient(v, True), int(raw.max()))
    elif variant in (R.LIGHT, R.LIGHT_INSHADER):
        ct = ob.precompute_gradient(ob.normalize_data(v))
    else:
        ct = ob.normalize_data(v)
    mask = win(hr.mask_vec4(20))
    dose = ob.normalize_data(hr.raw_to_vec4(hr.dose_raw(13, 20, 7)))
    tf0 = zero_prefix_tf(tf_res, zeros)
    tf1 = (zero_prefix_tf(2 * tf_res, 2 * zeros, 0.4)[0], hr.default_color_tf(2 * tf_res) * f32(0.5))
    vols = {R.VOLUME_MASK: [mask, dose, ct], R.THREE_FILES: [ct, dose, mask], R.MULTI_CTRT: [ct, dose],
            R.ILLUSTRATIVE: [ct, dose], R.TF_CALIB: [ct, mask]}.get(variant, [ct])
    return vols, [tf0, tf1] if variant in (R.VOLUME_MASK, R.THREE_FILES, R.MULTI_CTRT, R.ILLUSTRATIVE) else [tf0]


@functools.lru_cache(maxsize=None)
def scene(variant, kind="phantom"):
    if kind == "phantom":
        return vt.scene(variant, n=N)
    if kind == "thin":  # opacity tables scaled to top out at 0.002: 900 samples stay clear of the cut-offs
        vols, tfs = vt.scene(variant, n=N)
        return vols, [(hr.thin_opacity_tf(len(o), 0.002), c) for o, c in tfs]
    _, res, zeros = kind.split(":")  # "aniso:<tf res>:<zero prefix>"
    return aniso_scene(variant, int(res), int(zeros))


def cases(variant):
    """(id, scene kind, W, H, uniform keywords) for one variant."""
    step, count = stepping(N)
    base = dict(steps_count=count, step_size=step)
    out = [(f"cam-{c}", "phantom", W, H, {**base, **kw}) for c, kw in CAMERAS.items()]
    out += [
        ("clips", "phantom", W, H, {**base, "clip_x": (0.2, 0.1), "clip_y": (0.05, 0.0), "clip_z": (0.0, 0.3)}),
        ("varstep-jitter", "phantom", W, H, {**base, "toggles": (1, 1, 0, 0), "yaw": 2.0, "pitch": -0.4}),
        ("jitter", "phantom", W, H, {**base, "toggles": (0, 1, 0, 0)}),
        ("short-7", "phantom", W, H, {**base, "steps_count": 7}),
        ("steps-0", "phantom", W, H, {**base, "steps_count": 0}),
        ("steps-1", "phantom", W, H, {**base, "steps_count": 1}),
        # 900 variable steps of ~1/500 where every decision is a cut-off or a box face.  Shaders that also decide on
        # sampled fields (a mask, a gradient of zero length, central differences over 1/500) keep the fixed step:
        # a ray that samples a field 900 times puts some sample within the position error of such a boundary on
        # more than FRAGILE_MAX of the pixels
        ("steps-900", "thin", W, H, {**base, "steps_count": 900, "toggles": (
            1 if variant in (R.BASIC, R.LIGHT, R.THREE_FILES, R.MULTI_CTRT) else 0, 0, 0, 0)}),
        ("aniso-tf16", "aniso:16:3", W, H, {**base, "yaw": 1.0, "pitch": 0.5}),
        ("aniso-tf64", "aniso:64:8", W, H, {**base, "yaw": 2.0, "pitch": -0.4}),
        ("aniso-tf257", "aniso:257:30", W, H, {**base, "distance": 0.7, "yaw": 1.0}),
    ]
    if variant != R.ILLUSTRATIVE:  # the production step 1 / n, where no exact tie decides the frame
        s1, c1 = hr.stepping_params(N, N, N)
        out.append(("step-1/n", "phantom", W, H, dict(steps_count=c1, step_size=s1)))
    return out


def all_cases():
    return [(v, *c) for v in range(8) for c in cases(v)]


def case_ids():
    return [f"{ob_name(v)}-{c[0]}" for v in range(8) for c in cases(v)]


def ob_name(v):
    return ["BASIC", "LIGHT", "VOLUME_MASK", "THREE_FILES", "MULTI_CTRT", "TF_CALIB", "ILLUSTRATIVE",
            "LIGHT_INSHADER"][v]


def uniforms(W_, H_, kw):
    return hr.make_uniforms(W_, H_, **kw)


@functools.lru_cache(maxsize=None)
def reference(variant, cid, mutant=None):
    kind, W_, H_, kw = next((k, w, h, a) for i, k, w, h, a in cases(variant) if i == cid)
    vols, tfs = scene(variant, kind)
    return R.render(variant, uniforms(W_, H_, kw), vols, tfs, W_, H_, mutant=mutant)


def inputs(variant, cid):
    kind, W_, H_, kw = next((k, w, h, a) for i, k, w, h, a in cases(variant) if i == cid)
    vols, tfs = scene(variant, kind)
    return uniforms(W_, H_, kw), vols, tfs, W_, H_
