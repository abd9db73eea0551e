"""Seeded random cases for the five feature marches (projections, isosurface, shadows, surface output, ray bounds), shared by
tests/test_random_features.py (restatements against the oracle) and tests/test_random_features_gpu.py (kernels against the
restatements): non-cubic noise volumes, ragged viewports, random cameras (inside the box included), clips, stepping, table shapes
and every family's own parameters.  cases(seed)[index] replays one case.  Harness only."""
import numpy as np

import bound_ref as br
import host_ref as hr
import iso_ref as ir
import oracle_binding as ob
import proj_ref as pr
import shadow_ref as shr
import surf_ref as sr

f32 = np.float32
BASIC, LIGHT, MIP, MINIP, AVERAGE, ISO = 0, 1, 8, 9, 10, 11
FAMILIES = ("proj", "iso", "shadow", "surf", "bound")
SEEDS = range(6)
CASES_PER_SEED = 20
SIDES = [5, 7, 9, 13, 16, 20, 23]  # per axis, independently: brick grids that are neither cubic nor whole
ZERO_BELOW = 2500  # of 4096 raw levels
HOSTILE = [np.nan, np.inf, -np.inf, -1.0, 2.0]


class Case:
    """One draw.  `draw` holds every scalar of it (what a failure message prints); the arrays are vec4 [nz, ny, nx, 4], tf =
    (opacity, colour), near / far = float32 [H, W] depth planes or None."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def uniforms(self, **over):
        kw = dict(self.kw)
        kw.update(over)
        return hr.make_uniforms(self.W, self.H, **kw)


def steep_tf(res, gain=4.0):
    """The dedicated tests' steep ramp: opacity min(1, gain * ramp), exactly 0 at density 0."""
    return np.minimum(hr.default_opacity_tf(res) * f32(gain), f32(1.0)).astype(f32), hr.default_color_tf(res)


def flat_tf(res, rgb=(0.8, 0.55, 0.3)):
    """Constant colour, opacity 1 everywhere (tests/test_isosurface.py): LIGHT's first in-box sample is opaque."""
    return np.ones(res, f32), np.tile(np.array([*rgb, 1.0], f32), (res, 1))


def edge_volume():
    """20 x 13 x 16 voxels for the refinement's edges (ISO and the surface output): exact-zero air around a block of density 0.9, a
    plate of NaN voxels on the block's -x face (a ray that comes through it hits the block with d_prev = NaN: t is NaN, outside
    [0, 1], and q = p_k), the gradient of all that in .rgb but exactly zero in the upper half z >= 8 (a hit there has a NaN normal:
    the ambient term only).  With edge_clip the clip box begins inside the block: rays from -y hit on their first in-box step."""
    v = np.zeros((16, 13, 20, 4), f32)
    v[4:12, 3:10, 6:14, 3] = f32(0.9)
    v[4:12, 3:10, 5, 3] = np.nan
    v = ob.precompute_gradient(v)
    v[8:, :, :, :3] = f32(0.0)
    return v


edge_clip = dict(clip_y=(0.5, 0.0))


def depth_planes(rng, u, W, H):
    """(mode, hostile, near, far): planes drawn between the depths of the box's corners, a few hostile values mixed into a quarter
    of the cases (NaN, +-inf, -1, 2: tests/test_ray_bounds_gpu.hostile's values)."""
    lo, hi = br.box_corner_depths(u)
    mode = str(rng.choice(["near", "far", "both"], p=[0.25, 0.45, 0.3]))
    hostile = bool(rng.random() < 0.25)
    planes = []
    for _ in range(2):
        with np.errstate(all="ignore"):
            p = (f32(lo) + (f32(hi) - f32(lo)) * rng.random((H, W), dtype=np.float32)).astype(f32)
        if hostile:
            bad = rng.random((H, W)) < 0.06
            p[bad] = np.array(HOSTILE, f32)[rng.integers(0, len(HOSTILE), size=int(bad.sum()))]
        planes.append(p)
    return mode, hostile, planes[0] if mode != "far" else None, planes[1] if mode != "near" else None


def tie_depths(case, u, rng, count=3000):
    """(pixels (N, 2), depths (N,)): for some of `count` seeded rays, a depth d whose S = sigma(g(d)) equals sigma(p_k) of one of the
    ray's first in-box steps EXACTLY -- where the definition's >= (near) and < (far) part company from > and <=.  p_k from
    surf_ref's positions, sigma and g from bound_ref; d by bisection over the float32 values in [0, 1] (S grows with d), kept only
    where the equality is exact (about one ray in seventy: near depth 1 one ulp of d moves S by many of its own)."""
    W, H = case.W, case.H
    none = np.zeros((0, 2), np.int64), np.zeros(0, f32)
    pix = np.stack([rng.integers(0, W, count), rng.integers(0, H, count)], 1)
    s = sr.march(u, W, H, case.vec4, case.tf[0], 0.5, pixels=pix, positions=True)
    if "positions" not in s:
        return none
    ray = np.nonzero(s["rayhit"])[0]
    P = s["positions"][:, ray]
    lo, hi = shr.clip_box(u)
    with np.errstate(all="ignore"):
        inb = np.all((P >= lo) & (P <= hi), axis=2)
    ok = inb.any(axis=0)
    k = np.minimum(np.argmax(inb, axis=0) + rng.integers(0, 4, size=ray.size), P.shape[0] - 1)
    ray, P, k = ray[ok], P[:, ok], k[ok]
    if ray.size == 0:
        return none
    pk = P[k, np.arange(ray.size)]
    rays = [ob.setup_ray(u, W, H, int(x), int(y)) for x, y in pix[ray]]
    start, end = np.array([r[1] for r in rays], f32), np.array([r[2] for r in rays], f32)
    with np.errstate(all="ignore"):  # (the direction as bound_ref.march normalises it)
        diff = end - start
        ln = np.sqrt((diff[:, 0] * diff[:, 0] + diff[:, 1] * diff[:, 1]) + diff[:, 2] * diff[:, 2])
        dr = (diff * (f32(1.0) / ln)[:, None]).astype(f32)
    target = br.sigma(pk, dr)
    px, py = pix[ray, 0], pix[ray, 1]

    def S(bits):
        return br.sigma(br.g(u, W, H, px, py, bits.astype(np.uint32).view(f32)), dr)

    a, b = np.zeros(ray.size, np.int64), np.full(ray.size, int(np.array(1.0, f32).view(np.uint32)), np.int64)
    for _ in range(32):
        m = (a + b) // 2
        with np.errstate(all="ignore"):
            ge = S(m) >= target
        a, b = np.where(ge, a, m + 1), np.where(ge, m, b)
    found, d = np.zeros(ray.size, bool), np.zeros(ray.size, np.int64)
    for off in (0, 1, -1, 2, -2):
        cand = np.clip(b + off, 0, None)
        with np.errstate(all="ignore"):
            eq = (S(cand) == target) & ~found
        d[eq] = cand[eq]
        found |= eq
    return pix[ray[found]], d[found].astype(np.uint32).view(f32)


def random_case(rng):
    nx, ny, nz = (int(x) for x in rng.choice(SIDES, size=3))
    W, H = int(rng.integers(17, 150)), int(rng.integers(17, 110))
    raw = rng.integers(0, 4096, size=(nz, ny, nx)).astype(np.uint16)
    zeroed = bool(rng.random() < 0.5)
    if zeroed:  # exact-zero air: something for the skipping forms to skip
        raw[raw < ZERO_BELOW] = 0
    vec4 = ob.precompute_gradient(ob.normalize_data(hr.raw_to_vec4(raw)))
    tf_res = int(rng.choice([16, 64, 257]))
    steep = bool(rng.random() < 0.5)
    tf = steep_tf(tf_res) if steep else (hr.default_opacity_tf(tf_res), hr.default_color_tf(tf_res))
    n = max(nx, ny, nz)
    # (the camera, clips and stepping of test_random_gpu.random_case; the weights keep two cases in three non-trivial)
    steps = int(rng.choice([0, 1, 7, int(np.sqrt(3) * n), 3 * n, 900], p=[.04, .06, .1, .4, .3, .1]))
    kw = dict(steps_count=steps, step_size=float(rng.choice([1.0 / n, 0.37 / n, 1.0 / 900], p=[.5, .35, .15])),
              distance=float(rng.choice([0.27, 0.5, 0.8, 1.2, 3.0], p=[.08, .23, .23, .23, .23])), yaw=float(rng.uniform(-3.2, 3.2)),
              pitch=float(rng.uniform(-1.5, 1.5)), toggles=(int(rng.integers(0, 2)), int(rng.integers(0, 2)), 0, 0))
    if rng.random() < 0.5:
        kw.update(clip_x=(float(rng.uniform(0, 0.4)), float(rng.uniform(0, 0.4))), clip_y=(float(rng.uniform(0, 0.3)), 0.0),
                  clip_z=(0.0, float(rng.uniform(0, 0.45))))
    if rng.random() < 0.5:
        kw.update(light_pos=(float(rng.uniform(-3, 3)), float(rng.uniform(-3, 3)), float(rng.uniform(-3, 3)), 1.0))
    c = Case(nx=nx, ny=ny, nz=nz, W=W, H=H, vec4=vec4, tf=tf, kw=kw, zeroed=zeroed, tf_res=tf_res, steep=steep,
             proj_variant=int(rng.choice([MIP, MINIP, AVERAGE])),
             iso=float(rng.choice([0.3, 0.45, 0.6, 0.75])),
             surf_variant=int(rng.choice([BASIC, LIGHT, LIGHT, ISO])),
             tau=float(rng.choice([0.0, 0.25, 0.5, 0.9, float(sr.TAU_BASIC), float(sr.TAU_LIGHT)])),
             shadow_divisor=int(rng.choice([1, 2, 4, 8])), shadow_scale=float(rng.choice([0.0, 0.5, 1.0, 4.0], p=[.2, .2, .4, .2])),
             bound_variant=int(rng.choice([BASIC, LIGHT])))
    c.bound_mode, c.bound_hostile, c.near, c.far = depth_planes(rng, c.uniforms(), W, H)
    # exact ties in six cases of ten, from a generator of their own (the main sequence does not depend on them)
    ties = np.random.default_rng([W, H, nx, ny, nz, steps])
    c.bound_ties = 0
    if ties.random() < 0.6:
        for plane in (c.near, c.far):
            if plane is not None:
                pix, d = tie_depths(c, c.uniforms(), ties)
                plane[pix[:, 1], pix[:, 0]] = d
                c.bound_ties += len(d)
    c.draw = dict(volume=(nx, ny, nz), W=W, H=H, zeroed=zeroed, tf_res=tf_res, steep=steep, kw=kw, proj_variant=c.proj_variant,
                  iso=c.iso, surf_variant=c.surf_variant, tau=c.tau, shadow=(c.shadow_divisor, c.shadow_scale),
                  bound=(c.bound_variant, c.bound_mode, c.bound_hostile, c.bound_ties))
    return c


def cases(seed):
    """The cases of one seed, each with .seed and .index."""
    rng = np.random.default_rng(3000 + seed)
    out = [random_case(rng) for _ in range(CASES_PER_SEED)]
    for i, c in enumerate(out):
        c.seed, c.index = seed, i
    return out


def light_volume(case, u, scale=None, fused=False):
    """The restated light volume of the case's divisor under uniforms u, in either arithmetic mode."""
    lo, hi = shr.clip_box(u)
    return shr.build(case.vec4, case.tf[0], case.shadow_divisor, case.shadow_scale if scale is None else scale, list(u.light_pos)[:3],
                     lo, hi, fused=fused)


def reference(case, family, u=None, fused=False):
    """(frag [H, W, 4], composited, covered) of the family's restatement with the case's parameters under uniforms u (default: the
    case's own; a batch passes its other cameras), in separately rounded or fused arithmetic."""
    u = case.uniforms() if u is None else u
    W, H = case.W, case.H
    if family == "proj":
        return pr.frame(case.proj_variant, u, W, H, case.vec4, case.tf, fused=fused)
    if family == "iso":
        return ir.frame(u, W, H, case.vec4, case.tf, case.iso, fused=fused)
    if family == "shadow":
        return shr.frame(u, W, H, case.vec4, case.tf, light_volume(case, u, fused=fused), fused=fused)
    if family == "surf":
        if case.surf_variant == ISO:
            return sr.iso_frame(u, W, H, case.vec4, case.tf, case.iso, fused=fused)
        return sr.frame(u, W, H, case.vec4, case.tf[0], case.tau, fused=fused)
    if family == "bound":
        return br.frame(case.bound_variant, u, W, H, case.vec4, case.tf, case.near, case.far, fused=fused)
    raise ValueError(family)


def acts(case, family, ref, plain):
    """Whether the feature acts in `ref` = reference(case, family): composited > 0 and the family's own condition, judged on the
    restatements alone.  plain = {BASIC: (frag, composited, covered), LIGHT: ...} of the same uniforms without the feature."""
    frag, n, cov = ref
    if n <= 0:
        return False
    if family in ("iso", "surf"):
        return cov > 0  # (covered = pixels with a hit)
    if family == "bound":
        return n < plain[case.bound_variant][1]
    if family == "shadow" and case.shadow_scale > 0:
        return not np.array_equal(np.asarray(frag, f32).view(np.uint32), np.asarray(plain[LIGHT][0], f32).view(np.uint32))
    return True
