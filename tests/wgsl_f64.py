"""Float64 restatement of the eight fragment shaders, written from the WGSL, as a reference that is independent of the
C oracle (oracle/vr_oracle.c) and of every kernel form.

Each fragment is computed from its definition in double precision, with no operation order copied from the f32 code:
an eye ray through the pixel centre is cut by the proxy box, every sample position is start + k * step (no repeated
additions), the samplers use exact trilinear / linear weights, and the per-sample body follows the variant's fs_main.
Citations are paths below the reference's App/shaders/ directory.  Alongside each fragment the march records whether
any discrete decision came close to its threshold (`fragile`); `judge` leaves such pixels out of the value check.

Inputs come from host_ref (uniforms, tables) and from volumes already prepared in f32; `normalize_data` and
`precompute_gradient` below are the f64 statements of the host preparation (App/src/file/VolumeFile.cpp).

CONVENTIONS the WGSL does not fix, and why:
  * normalize(vec3(0)) shades with the ambient term only.  WGSL leaves normalize(0) undefined; on the reference's
    platforms N.L is NaN and max(NaN, 0) is 0, so the diffuse term drops out and dst stays finite.
  * pow(x, y) is exp2(y * log2(x)), the expansion WGSL specifies, so pow(0, 0) = exp2(0 * -inf) is NaN.  ILLUSTRATIVE
    meets it when a zero-gradient sample lies where the texture-space distance has clamped to 1 (air far behind the
    entry face); the NaN then stays in dst.  Frames are compared NaN pattern for NaN pattern.
  * The jitter hash fract(sin(dot(xy, (12.9898, 78.233))) * 43758.5453) amplifies the last bit of sin by 4e4, so no
    restatement at another precision can reproduce it.  Its value is taken from oracle_binding.jitter: this is the one
    input this module takes from the oracle.
  * Hardware filtering with 8-bit fixed-point weights is not modelled: WebGPU does not require it and the HIP kernels
    compute the weights in f32.
"""
from __future__ import annotations

import numpy as np

from oracle_binding import jitter

BASIC, LIGHT, VOLUME_MASK, THREE_FILES, MULTI_CTRT, TF_CALIB, ILLUSTRATIVE, LIGHT_INSHADER = range(8)

f64 = np.float64
# proxy box in world space, Application.h:147-156; uvw = (x + .5, y + .5, .5 - 2 z)
BOX_MIN = np.array([-0.5, -0.5, -0.25])
BOX_MAX = np.array([0.5, 0.5, 0.25])

# ------------------------------------------------------------------------------------------ tolerances (one place)
# Where the f32 march can sit, relative to the exact one.  Unit roundoff u = 2^-24 ~ 6.0e-8.
#  * Ray set-up: the f32 view ray is the difference of the un-projected near and far points; the far point lies up to
#    `far` = 100 away, where one ulp is 7.6e-6, so the direction carries ~1e-7 and the entry point (~1 away) a few ulp
#    of its coordinates.  The largest entry / exit error the f32 set-up shows over this suite's cameras is 1.2e-6;
#    POS0 = 2.5e-6 (uvw units) covers it twice over.
#  * Marching: p += step rounds each coordinate of a sample that can blend (p <= 1) to within half an ulp of 1,
#    ADD_ERR = 2^-25; the step vector dir * step carries STEP_ULPS = 4 roundings of its own length (normalize, the
#    product, the variable-step division).
#  So after k steps a sample lies within pos_err(k) = POS0 + k * (ADD_ERR + STEP_ULPS * u * |step|) of the exact
#  position on every axis.
# A value read through the sampler moves with its position: a trilinear sample changes by at most the largest
# neighbour difference of the volume per texel of travel on each axis, and a TF lookup by the largest neighbour
# difference of the table times its resolution per unit of density.  GRAD is the product of the two, taken over every
# channel of the volumes whose values the shader blends and every table it reads (`lipschitz`, computed from the
# inputs, never set per case), so a sample moves by at most 3 * pos_err * n * GRAD (three axes, n texels per unit).  Front-to-back weights sum to
# at most 1, so each blended quantity inherits that change once; the colour is further scaled by the shading factor,
# at most kD * diffuse + kA * ambient = 3.5 + 0.5 for the scenes here (SHADE).  The rounding of the few dozen f32
# operations of one sample (interpolations, shading, blend) adds ACC_ULPS * u per step.  Hence
#     alpha_tol(k, n) = 3 * pos_err(k) * n * GRAD + k * ACC_ULPS * u       (dst.a, and any opacity-only quantity)
#     atol(k, n)      = SHADE * alpha_tol(k, n)                             (every channel of the frame)
# at k = steps_count.  For the suite's 16..32-texel scenes this is 6e-4..1.2e-3, above BASELINE.json's 1e-4 ceiling
# because it is a bound (linear drift, the steepest edge, the brightest light all at once), not an estimate.  What
# the frames actually show is reported (`Verdict.max_err`): below 7e-5 on those scenes, about 1e-3 at C3 / C4 size
# (886 steps of 1/512), where the bound is 0.12.
POS0 = 2.5e-6
ADD_ERR = 2.0 ** -25
STEP_ULPS = 4
SHADE = 4.0
ACC_ULPS = 16
U32 = 2.0 ** -24
# Decisions: a pixel is FRAGILE when one of its decisions comes within the error of its operand:
#  * position tests (in-box and clip planes, mask > 0, the nearest-sampled mask) within FRAG_SAFETY * pos_err(k) of
#    where their outcome changes;
#  * the dst.a <= 0.95 cut-off within alpha_tol of 0.95;
#  * a gradient shorter than GRAD_EPS, where normalize() turns the sampler's rounding and position error into a
#    different direction (and at 0 into the ambient-only rule);
#  * ILLUSTRATIVE's distance clamp at 1 on a zero gradient, where pow(0, 0) = NaN and pow(0, y > 0) = 0 part.
# A decision only counts where the sample would blend something (nonzero or non-finite opacity, ray still open).
# The dst.a < 1.0 cut-off is no decision in this sense: where the f32 march may stop early, 1 - dst.a is within
# alpha_tol, and the light still to come is at most (1 - dst.a) * SHADE, inside atol.
FRAG_SAFETY = 2.0
GRAD_EPS = 1e-3
# Frame-level limits: at most FRAGILE_MAX of the covered pixels may be fragile; rays that pass within GRAZE (world
# units, ten times POS0) of the box's surface or of the near plane may differ in coverage.
FRAGILE_MAX = 0.01
GRAZE = 4e-5


def pos_err(k, step):
    return POS0 + np.asarray(k, dtype=f64) * (ADD_ERR + STEP_ULPS * U32 * np.abs(step))


def alpha_tol(steps, step, n, grad):
    return 3.0 * float(np.max(pos_err(steps, step))) * n * grad + steps * ACC_ULPS * U32


def atol(steps, step, n, grad):
    """Largest |f32 - f64| a covered, non-fragile pixel may show after `steps` samples of length `step` (the largest
    of the frame), n = the largest texel count per unit of any volume the shader reads, grad = `lipschitz` of its
    inputs.  Derivation above."""
    return SHADE * alpha_tol(steps, step, n, grad)


def _neighbour_diff(v, channels, chunk=16):
    """Largest |difference| of face neighbours over `channels`, in slabs of z so that a large volume is never
    widened whole."""
    m = 0.0
    for z0 in range(0, v.shape[0], chunk):
        s = np.asarray(v[z0:z0 + chunk + 1, ..., channels], dtype=np.float32)
        for ax in range(3):
            if s.shape[ax] > 1:
                m = max(m, float(np.abs(np.diff(s, axis=ax)).max()))
    return m


def lipschitz(volumes, tfs):
    """GRAD: largest neighbour difference of the blended channels times the largest slope of the tables (at least 1,
    for a channel used as it is).  volumes: [(vec4 array, channels)]."""
    dv = max(_neighbour_diff(v, ch) for v, ch in volumes)
    slope = max(max(float(np.abs(np.diff(np.asarray(t, dtype=f64), axis=0)).max(initial=0.0)) * len(t)
                    for t in pair) for pair in tfs)
    return dv * max(1.0, slope)


# ------------------------------------------------------------------------------------------ samplers (WebGPU)

def _axis(c, n):
    """Linear filter along one axis, clamp-to-edge: texel centres at (i + 1/2) / n."""
    x = c * n - 0.5
    x0 = np.floor(x)
    f = x - x0
    i0 = np.clip(x0, 0, n - 1).astype(np.int64)
    i1 = np.clip(x0 + 1, 0, n - 1).astype(np.int64)
    return i0, i1, f


class Volume:
    """vec4 texels, array shape (nz, ny, nx, 4), texel (i, j, k) at [k, j, i] (VolumeFile.cpp:306).  f32 storage is
    read per corner and widened, so a 2 GiB volume is never copied."""

    def __init__(self, vec4, half_texel=False):
        self.v = vec4
        self.nz, self.ny, self.nx = vec4.shape[:3]
        self.shift = 0.5 if half_texel else 0.0  # mutant hook: texel centres at i / n

    def linear(self, p):
        """textureSample(t, samplerLin, p) (Sampler.cpp:9-16: linear, clamp-to-edge): (N, 4) f64."""
        i0, i1, fx = _axis(p[:, 0] + self.shift / self.nx, self.nx)
        j0, j1, fy = _axis(p[:, 1] + self.shift / self.ny, self.ny)
        k0, k1, fz = _axis(p[:, 2] + self.shift / self.nz, self.nz)
        out = np.zeros((p.shape[0], 4))
        for k, wz in ((k0, 1.0 - fz), (k1, fz)):
            for j, wy in ((j0, 1.0 - fy), (j1, fy)):
                for i, wx in ((i0, 1.0 - fx), (i1, fx)):
                    out += (wx * wy * wz)[:, None] * self.v[k, j, i].astype(f64)
        return out

    def nearest(self, p):
        """textureSample(t, samplerNN, p) (Sampler.cpp:18-24): texel floor(p * n), clamp-to-edge."""
        i = np.clip(np.floor(p[:, 0] * self.nx), 0, self.nx - 1).astype(np.int64)
        j = np.clip(np.floor(p[:, 1] * self.ny), 0, self.ny - 1).astype(np.int64)
        k = np.clip(np.floor(p[:, 2] * self.nz), 0, self.nz - 1).astype(np.int64)
        return self.v[k, j, i].astype(f64)

    @property
    def n(self):
        return max(self.nx, self.ny, self.nz)


class TF:
    """1-D opacity (R) and colour (R, 4) tables sampled linearly with clamp-to-edge at coordinate d."""

    def __init__(self, opacity, color, half_texel=False):
        self.o = np.asarray(opacity, dtype=f64)
        self.c = np.asarray(color, dtype=f64)[:, :3]
        self.shift = 0.5 if half_texel else 0.0

    def _lookup(self, table, d):
        n = table.shape[0]
        i0, i1, f = _axis(d + self.shift / n, n)
        if table.ndim == 2:
            f = f[:, None]
        return table[i0] * (1.0 - f) + table[i1] * f

    def opacity(self, d):
        return self._lookup(self.o, d)

    def color(self, d):
        return self._lookup(self.c, d)


# ------------------------------------------------------------------------------------------ small vector helpers

def _dot(a, b):
    return np.sum(a * b, axis=-1)


def _length(a):
    return np.sqrt(_dot(a, a))


def _normalize0(a):
    """normalize(a), with the zero vector mapped to zero (see CONVENTIONS): then N.L = 0 and only ambient remains."""
    n = _length(a)
    safe = np.where(n > 0, n, 1.0)
    return np.where((n > 0)[:, None], a / safe[:, None], 0.0)


def _wgsl_pow(x, y):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.exp2(y * np.log2(x))


def _blinn_phong(N, w, lpos, diffuse, ambient, kD, kA):
    """light.diffuse * max(dot(N, L), 0) * kD + light.ambient * kA, L = normalize(lightPos - w)."""
    L = _normalize0(lpos[None, :] - w)
    m = np.maximum(_dot(N, L), 0.0)
    return diffuse[None, :] * (m * kD)[:, None] + ambient[None, :] * kA


# ------------------------------------------------------------------------------------------ ray set-up

def _m(field):
    """Column-major 4x4 uniform -> row-major matrix."""
    return np.array(field[:], dtype=f64).reshape(4, 4).T


def _slab(eye, d, lo, hi):
    with np.errstate(divide="ignore", invalid="ignore"):
        ta = (lo[None, :] - eye[None, :]) / d
        tb = (hi[None, :] - eye[None, :]) / d
    tn, tf = np.minimum(ta, tb), np.maximum(ta, tb)
    tn = np.where(d == 0, np.where((eye >= lo) & (eye <= hi), -np.inf, np.inf), tn)
    tf = np.where(d == 0, np.where((eye >= lo) & (eye <= hi), np.inf, -np.inf), tf)
    return tn.max(axis=1), tf.min(axis=1), tn.argmax(axis=1), tf.argmin(axis=1)


def eye_rays(u, W, H, pxy):
    """For pixels pxy (N, 2): (hit, graze, P0, P1) in world space.  The fragment of the proxy box's front face exists
    iff the eye ray through the pixel centre enters the box between the near and far planes (front faces, cull back,
    Application.cpp:589-590; WebGPU clip volume 0 <= z <= w).  The entry and exit coordinates of the faces that are hit
    are vertex constants, so they are snapped onto those faces exactly."""
    proj, view_inv = _m(u.proj), _m(u.view_inv)
    eye = np.array(u.camera_pos[:], dtype=f64)
    px, py = pxy[:, 0].astype(f64), pxy[:, 1].astype(f64)
    ndcx = 2.0 * (px + 0.5) / W - 1.0
    ndcy = 1.0 - 2.0 * (py + 0.5) / H
    dv = np.stack([ndcx / proj[0, 0], ndcy / proj[1, 1], -np.ones_like(ndcx)], axis=1)
    d = dv @ view_inv[:3, :3].T
    d /= np.linalg.norm(d, axis=1)[:, None]
    fwd = -view_inv[:3, 2] / np.linalg.norm(view_inv[:3, 2])
    near = proj[2, 3] / (proj[2, 2] - 1.0)  # glm::perspective: P[2][2] = -(f+n)/(f-n), P[2][3] = -2fn/(f-n)
    far = proj[2, 3] / (proj[2, 2] + 1.0)

    def hits(grow):
        t0, t1, a0, a1 = _slab(eye, d, BOX_MIN - grow, BOX_MAX + grow)
        depth = t0 * (d @ fwd)
        return (t0 < t1) & (depth >= near - grow) & (depth <= far), t0, t1, a0, a1

    hit, t0, t1, a0, a1 = hits(0.0)
    graze = hits(GRAZE)[0] != hits(-GRAZE)[0]
    P0 = eye[None, :] + d * t0[:, None]
    P1 = eye[None, :] + d * t1[:, None]
    r = np.arange(len(d))
    P0[r, a0] = np.where(d[r, a0] > 0, BOX_MIN[a0], BOX_MAX[a0])
    P1[r, a1] = np.where(d[r, a1] > 0, BOX_MAX[a1], BOX_MIN[a1])
    return hit, graze, P0, P1


def _uvw(P):
    return np.stack([P[:, 0] + 0.5, P[:, 1] + 0.5, 0.5 - 2.0 * P[:, 2]], axis=1)


# ------------------------------------------------------------------------------------------ fs_main

LIGHT_CONSTS = {  # kD, kA of each shader's BlinnPhong
    LIGHT: (2.5, 0.5),           # BasicVolLightApp.wgsl:137-147
    LIGHT_INSHADER: (2.5, 0.5),
    VOLUME_MASK: (1.5, 0.5),     # VolumeMaskApp.wgsl:116-123 (own light position and colours)
    MULTI_CTRT: (3.5, 0.5),      # MultiCTRTApp.wgsl:129-139
    ILLUSTRATIVE: (3.5, 0.5),    # MutliCTRTIllustrative.wgsl:132-143
}
# world-step z scale of CalculateWorldStep, and whether it is taken before the variable-step override
WORLD_STEP = {LIGHT: (0.5, True), LIGHT_INSHADER: (0.5, True),         # BasicVolLightApp.wgsl:78-84, 184-185
              MULTI_CTRT: (0.7, False), ILLUSTRATIVE: (0.7, False)}     # MultiCTRTApp.wgsl:154-160, 213-214
CUTOFF_095 = {BASIC, MULTI_CTRT, ILLUSTRATIVE, TF_CALIB}                # `dst.a <= 0.95`; the rest `dst.a < 1.0`

MUTANTS = (
    "vol_half_texel", "tf_half_texel", "late_start", "steps_plus_one", "basic_cutoff_swapped",
    "light_world_step_after_override", "inshader_gradient_sign", "mask_r_only", "mask_tables_swapped",
    "rt_mix_swapped", "ctrt_no_gradient_modulation", "ctrt_kd_2_5", "illustrative_dist_unclamped",
    "illustrative_no_alpha_factor", "calib_mask_linear",
)


class Result:
    """frag (N, 4) f64; covered, graze, fragile (N,) bool; n_vol = largest texel count per unit of the volumes read;
    steps = the march's sample count (for the tolerance)."""

    def __init__(self, frag, covered, graze, fragile, n_vol, steps, grad, step=0.0):
        self.frag, self.covered, self.graze, self.fragile = frag, covered, graze, fragile
        self.n_vol, self.steps, self.grad, self.step = n_vol, steps, grad, step

    @property
    def atol(self):
        return atol(self.steps, self.step, self.n_vol, self.grad)

    def image(self, W, H):
        return Result(self.frag.reshape(H, W, 4), self.covered.reshape(H, W), self.graze.reshape(H, W),
                      self.fragile.reshape(H, W), self.n_vol, self.steps, self.grad, self.step)


def render(variant, u, volumes, tfs, W, H, pxy=None, mutant=None):
    """fs_main of `variant` for every pixel of a W x H frame (pxy None) or for the pixels pxy (N, 2).  volumes / tfs
    follow the slot tables of include/vr.h.  `mutant` names a deliberately wrong variant (MUTANTS) for the tests'
    self-check; None is the reference."""
    assert mutant is None or mutant in MUTANTS, mutant
    whole = pxy is None
    if whole:
        yy, xx = np.mgrid[0:H, 0:W]
        pxy = np.stack([xx.ravel(), yy.ravel()], axis=1)
    pxy = np.asarray(pxy).reshape(-1, 2)
    vols = [None if v is None else Volume(v, half_texel=(mutant == "vol_half_texel")) for v in volumes]
    tabs = [None if t is None else TF(t[0], t[1], half_texel=(mutant == "tf_half_texel")) for t in tfs]
    N = len(pxy)
    frag = np.zeros((N, 4))
    fragile = np.zeros(N, dtype=bool)
    hit, graze, P0, P1 = eye_rays(u, W, H, pxy)
    used = {BASIC: [0], LIGHT: [0], LIGHT_INSHADER: [0], VOLUME_MASK: [0, 1, 2], THREE_FILES: [0, 1],
            MULTI_CTRT: [0, 1], ILLUSTRATIVE: [0, 1], TF_CALIB: [0, 1]}[variant]
    n_vol = max(vols[i].n for i in used)
    # the channels whose values reach dst: densities, and the gradient that scales MULTI_CTRT / ILLUSTRATIVE opacity
    # (masks only select; a gradient that is normalised only turns the light, see GRAD_EPS)
    valued = {BASIC: [(0, [3])], LIGHT: [(0, [3])], LIGHT_INSHADER: [(0, [3])], TF_CALIB: [(0, [3])],
              VOLUME_MASK: [(1, [3]), (2, [3])], THREE_FILES: [(0, [3]), (1, [3])],
              MULTI_CTRT: [(0, [0, 1, 2, 3]), (1, [3])], ILLUSTRATIVE: [(0, [0, 1, 2, 3]), (1, [3])]}[variant]
    grad = lipschitz([(volumes[i], ch) for i, ch in valued], [t for t in tfs if t is not None])
    steps_count = int(u.steps_count)
    idx = np.nonzero(hit)[0]
    res = Result(frag, hit, graze, fragile, n_vol, steps_count, grad)
    if len(idx) == 0:
        return res.image(W, H) if whole else res
    P0, P1 = P0[idx], P1[idx]
    start, end = _uvw(P0), _uvw(P1)
    texC = np.stack([0.5 * P0[:, 0] + 0.5, -0.5 * P0[:, 1] + 0.5], axis=1)  # worldCoord.w == 1

    # SetupRay  BasicVolumeApp.wgsl:86-96
    diff = end - start
    ray_len = _length(diff)
    dirn = diff / ray_len[:, None]
    mode = int(u.fragment_mode)
    if mode in (1, 2, 3, 4):  # BasicVolumeApp.wgsl:128-143
        out = {1: np.abs(dirn), 2: start, 3: end, 4: np.concatenate([texC, np.zeros((len(idx), 1))], axis=1)}[mode]
        frag[idx, :3] = out
        frag[idx, 3] = 1.0
        return res.image(W, H) if whole else res

    step_size = np.full(len(idx), float(np.float32(u.step_size)))
    world_step = np.zeros((len(idx), 3))
    scale_z, before = WORLD_STEP.get(variant, (None, None))
    if mutant == "light_world_step_after_override" and variant in (LIGHT, LIGHT_INSHADER):
        before = False

    def calc_world_step(s):  # CalculateWorldStep
        return dirn * np.stack([s, s, -s * scale_z], axis=1)

    if before:
        world_step = calc_world_step(step_size)
    if int(u.toggles[0]) == 1:
        step_size = ray_len / steps_count  # GetStepSize, BasicVolumeApp.wgsl:62-65
    if scale_z is not None and not before:
        world_step = calc_world_step(step_size)
    if variant in (VOLUME_MASK, THREE_FILES):
        world_step = dirn * step_size[:, None]  # VolumeMaskApp.wgsl:213, ThreeFilesApp.wgsl:268: world += uvw step

    p0 = start.copy()
    if int(u.toggles[1]) == 1:  # :156-160, in.position.xy = pixel centre
        j = np.array([jitter(float(x) + 0.5, float(y) + 0.5) for x, y in pxy[idx]])
        p0 = p0 + dirn * (step_size * j)[:, None]
    if mutant == "late_start":
        p0 = p0 + dirn * (0.5 * step_size)[:, None]
    step = dirn * step_size[:, None]
    res.step = float(step_size.max())

    lo = np.array([0.0 + u.clip_x[0], 0.0 + u.clip_y[0], 0.0 + u.clip_z[0]], dtype=f64)
    hi = np.array([1.0 - u.clip_x[1], 1.0 - u.clip_y[1], 1.0 - u.clip_z[1]], dtype=f64)
    n_loop = steps_count + (1 if mutant == "steps_plus_one" else 0)
    # samples beyond the box exit never blend (the inside set of a line and a convex box is one interval); march to two
    # samples past the last exit so that the decisions next to it are still seen
    with np.errstate(divide="ignore", invalid="ignore"):
        t_exit = np.where(step > 0, (1.0 - p0) / step, np.where(step < 0, -p0 / step, np.inf)).min(axis=1)
    t_exit = np.where(np.isfinite(t_exit), t_exit, n_loop)
    n_loop = int(min(n_loop, max(0.0, np.ceil(t_exit.max())) + 2))

    cut095 = variant in CUTOFF_095
    if mutant == "basic_cutoff_swapped" and variant == BASIC:
        cut095 = False
    lpos = np.array(u.light_pos[:3], dtype=f64)
    ldif = np.array(u.light_diffuse[:3], dtype=f64)
    lamb = np.array(u.light_ambient[:3], dtype=f64)
    cam = np.array(u.camera_pos[:], dtype=f64)
    lp5 = np.array([0.0, -5.0, 0.0])
    dst = np.zeros((len(idx), 4))
    frg = np.zeros(len(idx), dtype=bool)
    snapped = int(u.toggles[1]) != 1 and mutant != "late_start"

    for k in range(n_loop):
        p = p0 + k * step
        wc = P0 + k * world_step
        e = FRAG_SAFETY * pos_err(k, step_size)[:, None]
        inside = np.all((p >= lo) & (p <= hi), axis=1)
        near_plane = np.minimum(np.abs(p - lo), np.abs(p - hi))
        if k == 0 and snapped:  # sample 0 lies on the entry face: both sides see that coordinate exactly
            near_plane = np.where(np.isin(p, (0.0, 1.0)), np.inf, near_plane)
        near_box = np.any(near_plane < e, axis=1)
        alive = (dst[:, 3] <= 0.95) if cut095 else (dst[:, 3] < 1.0)
        dec = np.zeros(len(idx), dtype=bool)  # a decision of this sample sits within its operand's error
        if cut095:
            dec |= np.abs(dst[:, 3] - 0.95) < alpha_tol(steps_count, step_size, n_vol, grad)
        g_vec = None  # the vector whose normalize() the shader takes

        if variant in (BASIC, LIGHT, LIGHT_INSHADER, TF_CALIB):  # BasicVolumeApp.wgsl:167-185 and relatives
            v = vols[0].linear(p)
            a = tabs[0].opacity(v[:, 3])
            c = tabs[0].color(v[:, 3])
            if variant == LIGHT:  # BasicVolLightApp.wgsl:210-228
                g_vec = v[:, :3]
            elif variant == LIGHT_INSHADER:  # ComputeGradient, BasicVolLightApp.wgsl:239-253 (enabled at :212)
                r = np.zeros((len(idx), 3))
                for ax in range(3):
                    dv = np.zeros(3)
                    dv[ax] = 1.0
                    dvs = dv[None, :] * step_size[:, None]
                    r[:, ax] = vols[0].linear(p + dvs)[:, 3] - vols[0].linear(p - dvs)[:, 3]
                l = _length(r)
                sign = 1.0 if mutant == "inshader_gradient_sign" else -1.0
                g_vec = np.where((l > 0)[:, None], sign * r / np.where(l > 0, l, 1.0)[:, None], 0.0)
                dec |= (l > 0) & (l < GRAD_EPS)
            if variant in (LIGHT, LIGHT_INSHADER):
                kD, kA = LIGHT_CONSTS[variant]
                c = c * _blinn_phong(_normalize0(g_vec), wc, lpos, ldif, lamb, kD, kA)
            if variant == TF_CALIB:  # TFCalibrationApp.wgsl:171-184: samplerNN mask overrides colour and opacity
                sample = vols[1].linear if mutant == "calib_mask_linear" else vols[1].nearest
                m = sample(p)[:, 0] > 0
                for ax in range(3):
                    for sg in (-1.0, 1.0):
                        q = p.copy()
                        q[:, ax] += sg * e[:, 0]
                        dec |= (sample(q)[:, 0] > 0) != m
                c = np.where(m[:, None], np.array([1.0, 1.0, 0.0])[None, :], c)
                a = np.where(m, 0.1, a)
        elif variant == VOLUME_MASK:  # VolumeMaskApp.wgsl:182-214; volumes 0 mask, 1 RT, 2 CT; tables 0 CT, 1 RT
            tct, trt = (tabs[1], tabs[0]) if mutant == "mask_tables_swapped" else (tabs[0], tabs[1])
            rt = vols[1].linear(p)[:, 3]
            ct = vols[2].linear(p)
            g_vec = ct[:, :3]
            kD, kA = LIGHT_CONSTS[VOLUME_MASK]
            c = tct.color(ct[:, 3]) * _blinn_phong(_normalize0(g_vec), wc, lp5, np.array([0.96, 0.76, 0.67]),
                                                    np.ones(3), kD, kA)
            a = tct.opacity(ct[:, 3])
            chans = 1 if mutant == "mask_r_only" else 3

            def masked(q):
                return np.any(vols[0].linear(q)[:, :chans] > 0, axis=1)

            m = masked(p)
            for ax in range(3):
                for sg in (-1.0, 1.0):
                    q = p.copy()
                    q[:, ax] += sg * e[:, 0]
                    dec |= masked(q) != m
            c = np.where(m[:, None], trt.color(rt), c)
            a = np.where(m, trt.opacity(rt), a)
        else:  # THREE_FILES (:224-269), MULTI_CTRT (:219-256), ILLUSTRATIVE (:271-310): volumes / tables 0 CT, 1 RT
            ct = vols[0].linear(p)
            rt = vols[1].linear(p)[:, 3]
            o_ct, c_ct = tabs[0].opacity(ct[:, 3]), tabs[0].color(ct[:, 3])
            o_rt, c_rt = tabs[1].opacity(rt), tabs[1].color(rt)
            if mutant == "rt_mix_swapped":
                o_rt = 1.0 - o_rt
            c = c_ct * (1.0 - o_rt)[:, None] + c_rt * o_rt[:, None]
            a = o_ct
            if variant in (MULTI_CTRT, ILLUSTRATIVE):
                g_vec = ct[:, :3]
                kD, kA = LIGHT_CONSTS[variant]
                if mutant == "ctrt_kd_2_5":
                    kD = 2.5
                c = c * _blinn_phong(_normalize0(g_vec), wc, lp5, ldif, lamb, kD, kA)
                glen = _length(g_vec)
                if variant == MULTI_CTRT:  # GradinetMagnitudeOpacityModulation :148-151
                    a = o_ct if mutant == "ctrt_no_gradient_modulation" else o_ct * glen
                else:  # IllustrativeContextPreservingOpacity :158-186, texture-space distance option (:182)
                    L = _normalize0(lp5[None, :] - wc)
                    V = _normalize0(cam[None, :] - wc)
                    Hh = _normalize0(V + L)
                    s = 0.5 + 2.5 * _length(L * g_vec) + 1.0 * _wgsl_pow(_length(Hh * g_vec), 1.0)
                    dist = _length(p - start)
                    if mutant != "illustrative_dist_unclamped":
                        # pow(0, 0) = NaN against pow(0, y > 0) = 0: matters whatever the opacity
                        frg |= (np.abs(dist - 1.0) < e[:, 0]) & (glen < GRAD_EPS) & alive & (inside | near_box)
                        dist = np.minimum(dist, 1.0)
                    fade = 1.0 if mutant == "illustrative_no_alpha_factor" else (1.0 - dst[:, 3])
                    inner = _wgsl_pow(5.0 * s * (1.0 - dist) * fade, 0.8)
                    a = o_ct * _wgsl_pow(glen, inner)

        if g_vec is not None:
            glen = _length(g_vec)
            dec |= (glen > 0) & (glen < GRAD_EPS)
        # a decision matters where the ray is open, the sample may count as inside, and it blends something
        frg |= (dec | near_box) & alive & (inside | near_box) & ((a != 0) | ~np.isfinite(a))
        blend = inside & alive  # FrontToBackBlend  BasicVolumeApp.wgsl:98-104
        om = (1.0 - dst[:, 3])[:, None]
        src = np.concatenate([c * a[:, None], a[:, None]], axis=1)
        dst = np.where(blend[:, None], om * src + dst, dst)

    frag[idx] = dst
    fragile[idx] = frg
    return res.image(W, H) if whole else res


# ------------------------------------------------------------------------------------------ the comparator

class Verdict:
    def __init__(self):
        self.problems = []
        self.max_err = 0.0
        self.atol = 0.0
        self.fragile = 0
        self.covered = 0

    @property
    def ok(self):
        return not self.problems

    def __repr__(self):
        return (f"Verdict(max_err={self.max_err:.3g}, atol={self.atol:.3g}, fragile={self.fragile}/{self.covered}, "
                f"problems={self.problems})")


def judge(frame, covered, ref):
    """Judges an f32 frame (with its covered-pixel mask, or None to skip that check) against the f64 reference
    `ref` (a Result of the same pixels).  Every constant is the module's; nothing is set per case."""
    v = Verdict()
    frame = np.asarray(frame, dtype=f64)
    cov = ref.covered & ~ref.graze
    v.covered = int(ref.covered.sum())
    v.atol = ref.atol
    if covered is not None:
        bad = (np.asarray(covered, dtype=bool) != ref.covered) & ~ref.graze
        if bad.any():
            v.problems.append(f"coverage differs on {int(bad.sum())} non-grazing pixels")
    # nothing is drawn where no fragment exists
    if np.any(frame[~ref.covered & ~ref.graze] != 0):
        v.problems.append("values outside the covered pixels")
    v.fragile = int((ref.fragile & cov).sum())
    if v.covered and v.fragile > FRAGILE_MAX * v.covered:
        v.problems.append(f"{v.fragile} fragile pixels of {v.covered}")
    judged = cov & ~ref.fragile
    nan_f, nan_r = np.isnan(frame), np.isnan(ref.frag)
    if np.any((nan_f != nan_r)[judged]):
        v.problems.append(f"NaN pattern differs on {int(np.any(nan_f != nan_r, axis=-1)[judged].sum())} pixels")
    fin = ~nan_f & ~nan_r
    err = np.where(fin, np.abs(frame - ref.frag), 0.0)[judged]
    if err.size:
        v.max_err = float(err.max())
        if v.max_err > v.atol:
            v.problems.append(f"max |f32 - f64| {v.max_err:.3g} > atol {v.atol:.3g} on "
                              f"{int(np.any(err > v.atol, axis=-1).sum())} pixels")
    return v


def assert_matches(frame, covered, ref, what=""):
    v = judge(frame, covered, ref)
    assert v.ok, (what, v)
    return v


# ------------------------------------------------------------------------------------------ host data preparation

def normalize_data(vec4, normalization_value=0):
    """VolumeFile::NormalizeData (VolumeFile.cpp:165-184): .a /= the normalisation value; 0 selects the largest raw
    value, which the reader broadcast into every lane (GetMaxNumber; the raw data is integer)."""
    v = np.asarray(vec4, dtype=f64).copy()
    if normalization_value == 0:
        normalization_value = int(v[..., 0].max())
    v[..., 3] /= normalization_value
    return v


def precompute_gradient(vec4, norm_to_zero_one=False):
    """VolumeFile::PreComputeGradient (VolumeFile.cpp:196-257): rgb = -(a[+1] - a[-1]) / 2 per axis, 0 outside the
    grid; with norm_to_zero_one every component is divided by the largest gradient length."""
    v = np.asarray(vec4, dtype=f64).copy()
    a = np.pad(v[..., 3], 1)
    g = np.stack([-(a[1:-1, 1:-1, 2:] - a[1:-1, 1:-1, :-2]),
                  -(a[1:-1, 2:, 1:-1] - a[1:-1, :-2, 1:-1]),
                  -(a[2:, 1:-1, 1:-1] - a[:-2, 1:-1, 1:-1])], axis=-1) * 0.5
    if norm_to_zero_one:
        g /= np.sqrt(np.sum(g * g, axis=-1)).max()
    v[..., :3] = g
    return v
