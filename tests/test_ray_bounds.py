"""CPU side of the per-pixel ray bounds (vr_set_ray_bounds, include/vr.h, csrc/vr_bound.h): the float32 restatement in bound_ref.py is
pinned to the oracle -- with the trivial bounds near = 0, far = 1 its frames and counts are the oracle's BASIC / LIGHT bit for bit, and
a pixel whose far bound leaves the steps 0 .. m-1 is the same pixel of an oracle frame rendered with steps_count = m --, it obeys the
properties the definition implies, and the library declares, lists and exports the entry point and carries both arithmetic modes'
march_bound_kernel instances without scratch."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import bound_ref as br
import host_ref as hr
import oracle_binding as ob
import surf_ref as sr
import vrtest as vt
from test_surface import CASES, H, W, steep_tf, uniforms
from volumerendering_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import check_exec_regions as cer  # noqa: E402
from march_units import march_units  # noqa: E402

f32 = np.float32
VARIANTS = [(ob.BASIC, "basic"), (ob.LIGHT, "light")]
FIXED_STEP = [c for c in CASES if c[2].get("toggles", (0,))[0] != 1]  # (the variable step's size depends on steps_count)


def plane(value):
    return np.full((H, W), value, f32)


def centre_plane(u):
    """The depth of world (0, 0, 0): the plane through the box centre."""
    return plane(br.depth_of_world(u, (0.0, 0.0, 0.0)))


def seeded_depth(u, seed=11):
    """A seeded per-pixel depth between the depths of the nearest and the farthest box corner."""
    lo, hi = br.box_corner_depths(u)
    t = np.random.default_rng(seed).random((H, W), dtype=np.float32)
    return (lo + (hi - lo) * t).astype(f32)


@pytest.mark.parametrize("variant,vid", VARIANTS, ids=[v[1] for v in VARIANTS])
@pytest.mark.parametrize("cid,kind,over,hits", CASES, ids=[c[0] for c in CASES])
def test_trivial_bounds_are_the_oracles_frame(cid, kind, over, hits, variant, vid):
    """near = 0, far = 1 (the two depths the ray set-up itself unprojects) leave out no step: frame and composited count are the
    oracle's, bit for bit, on every pixel."""
    v = vt.make_volume(kind, 16, gradient=True)
    tf = steep_tf()
    u = uniforms(16, **over)
    ob.set_arithmetic(ob.SEPARATE)
    ref, n_ref, cov_ref = ob.render(variant, u, [v], [tf], W, H, nthreads=4)
    r = br.march(variant, u, W, H, v, tf, plane(0.0), plane(1.0))
    print(cid, vid, "composited", n_ref, "covered", cov_ref)
    assert int(r["composited"].sum()) == n_ref and int(r["covered"].sum()) == cov_ref
    assert np.array_equal(vt.bits(r["frag"].reshape(H, W, 4)), vt.bits(ref))
    assert not np.any(r["before_near"]) and np.all(r["before_far"][r["covered"]] == u.steps_count)
    if hits:
        assert n_ref > 0


@pytest.mark.parametrize("variant,vid", VARIANTS, ids=[v[1] for v in VARIANTS])
@pytest.mark.parametrize("cid,kind,over,hits", FIXED_STEP, ids=[c[0] for c in FIXED_STEP])
def test_far_bound_is_the_oracle_with_fewer_steps(cid, kind, over, hits, variant, vid):
    """A far bound in front of which the steps 0 .. m-1 lie gives the pixel of an oracle frame rendered with steps_count = m: one
    oracle frame for every m that occurs, every ray pixel compared.  Two depth buffers: the plane through the box centre and a
    seeded per-pixel depth between the nearest and the farthest box corner.  Where rays have steps to lose (steps_count >= 7: with
    no step or one step per ray a quarter of the rays cannot both lose one and keep one) the buffers must be non-trivial: at least
    a quarter of the ray pixels lose a step and at least a quarter keep one."""
    v = vt.make_volume(kind, 16, gradient=True)
    tf = steep_tf()
    u = uniforms(16, **over)
    ob.set_arithmetic(ob.SEPARATE)
    for name, far in (("plane", centre_plane(u)), ("seeded", seeded_depth(u))):
        r = br.march(variant, u, W, H, v, tf, None, far)
        ray = r["covered"]
        m = r["before_far"]
        assert np.all(r["prefix"])  # sigma never steps back across the bound: the steps in front of it are the first m
        lose, keep = int((m[ray] < u.steps_count).sum()), int((m[ray] > 0).sum())
        print(cid, vid, name, "ray pixels", int(ray.sum()), "lose a step", lose, "keep one", keep, "m", sorted(set(m[ray].tolist())))
        if u.steps_count >= 7:
            assert 4 * lose >= ray.sum() and 4 * keep >= ray.sum()
        want = np.zeros((W * H, 4), f32)
        want_n = np.zeros(W * H, np.int64)
        for mm in sorted(set(m[ray].tolist())):
            um = uniforms(16, **{**over, "steps_count": int(mm)})
            sel = np.nonzero(ray & (m == mm))[0]
            px, n_px = ob.render_pixels(variant, um, [v], [tf], W, H, r["pixels"][sel], nthreads=4)
            want[sel] = px
            want_n[sel] = n_px
        assert np.array_equal(vt.bits(r["frag"][ray]), vt.bits(want[ray]))
        assert not np.any(r["frag"][~ray])
        # (render_pixels reports the total of its pixels: compared per group of equal m)
        for mm in sorted(set(m[ray].tolist())):
            sel = ray & (m == mm)
            assert int(r["composited"][sel].sum()) == int(want_n[np.nonzero(sel)[0][0]])


@pytest.mark.parametrize("variant,vid", VARIANTS, ids=[v[1] for v in VARIANTS])
@pytest.mark.parametrize("cid,kind,over,hits", CASES, ids=[c[0] for c in CASES])
def test_far_bound_never_adds_and_a_plane_splits_a_thin_march(cid, kind, over, hits, variant, vid):
    """A far bound alone composites no more than the unbounded march, per pixel.  Under a thin opacity table (no ray reaches the
    cut-off) the same depth buffer D as near and as far splits the counts: n_near + n_far == n_unbounded per pixel."""
    v = vt.make_volume(kind, 16, gradient=True)
    u = uniforms(16, **over)
    for D in (centre_plane(u), seeded_depth(u, 5)):
        tf = steep_tf()
        free = br.march(variant, u, W, H, v, tf)
        far = br.march(variant, u, W, H, v, tf, None, D)
        assert np.all(far["composited"] <= free["composited"])
        thin = (hr.thin_opacity_tf(64), hr.default_color_tf(64))
        free = br.march(variant, u, W, H, v, thin)
        a = br.march(variant, u, W, H, v, thin, D, None)
        b = br.march(variant, u, W, H, v, thin, None, D)
        assert float(free["frag"][:, 3].max(initial=0.0)) < 0.95
        assert np.array_equal(a["composited"] + b["composited"], free["composited"])
        if hits:
            assert free["composited"].sum() > 0


ROUND_TRIP = [c for c in CASES if c[0] not in ("steps0", "steps1")]


@pytest.mark.parametrize("variant,vid", VARIANTS, ids=[v[1] for v in VARIANTS])
@pytest.mark.parametrize("cid,kind,over,hits", ROUND_TRIP, ids=[c[0] for c in ROUND_TRIP])
def test_round_trip_through_the_surface_depth(cid, kind, over, hits, variant, vid):
    """far = the depth of the tau = 0.5 surface frame: on every hit pixel the steps in front of the bound number k or k + 1, k the
    hit's step index (the surface point lies between p_{k-1} and p_k; the depth's and sigma's roundings decide about p_k itself), and
    the bounded alpha is at most the surface frame's .w (it blends a prefix of the same alpha line)."""
    v = vt.make_volume(kind, 16, gradient=True)
    tf = steep_tf()
    u = uniforms(16, **over)
    s = sr.march(u, W, H, v, tf[0], 0.5)
    D = sr.depth(s["frag"], u, 0.5).reshape(H, W)
    r = br.march(variant, u, W, H, v, tf, None, D)
    hit = s["hit"]
    assert hit.sum() > 0
    m, k = r["before_far"][hit], s["k"][hit]
    print(cid, vid, "hit pixels", int(hit.sum()), "exactly k", int((m == k).sum()), "k + 1", int((m == k + 1).sum()))
    assert np.all((m == k) | (m == k + 1))
    assert np.all(r["frag"][hit, 3] <= s["frag"][hit, 3])
    assert np.all(r["prefix"])


def test_hostile_bounds_clip_the_pixel_and_raise_nothing():
    """NaN and +-inf on either side (an infinite depth times the inverse projection's zeros is NaN), a far bound at -1 (the near
    plane: in front of the box) or at 2 (beyond the far plane the unprojection lands behind the camera: no sigma is below it), and
    near > far give what a fully clipped ray gives -- zeros, nothing composited, covered as ever.  The same two values as NEAR
    bounds exclude nothing by the same arithmetic: the frame is the unbounded one."""
    v = vt.make_volume("phantom", 16, gradient=True)
    tf = steep_tf()
    u = uniforms(16)
    lo, hi = br.box_corner_depths(u)
    for variant, _ in VARIANTS:
        free = br.march(variant, u, W, H, v, tf)
        assert free["composited"].sum() > 0
        clipped = [(plane(np.nan), None), (None, plane(np.nan)), (plane(np.nan), plane(np.nan)), (plane(np.inf), None),
                   (plane(-np.inf), None), (None, plane(np.inf)), (None, plane(-np.inf)), (None, plane(-1.0)), (None, plane(2.0)),
                   (plane(hi), plane(lo)), (plane(1.0), plane(0.0))]
        with np.errstate(all="raise", invalid="ignore", over="ignore"):
            for near, far in clipped:
                r = br.march(variant, u, W, H, v, tf, near, far)
                assert not np.any(r["frag"]) and not np.any(r["composited"])
                assert np.array_equal(r["covered"], free["covered"])
            for near in (plane(-1.0), plane(2.0)):
                r = br.march(variant, u, W, H, v, tf, near, None)
                assert np.array_equal(vt.bits(r["frag"]), vt.bits(free["frag"]))
                assert np.array_equal(r["composited"], free["composited"])


# ---- the library ----------------------------------------------------------------------------------------------------------

def test_abi_symbol():
    lib = capi.load()
    header = open(os.path.join(ROOT, "include", "vr.h")).read()
    assert re.search(r"\bint\s+vr_set_ray_bounds\s*\(\s*vr_ctx\s*\*\s*\w+\s*,\s*const\s+void\s*\*\s*d_near\s*,\s*const\s+void\s*\*\s*d_far\s*\)", header)
    assert "vr_set_ray_bounds" in capi.ABI_SYMBOLS
    assert hasattr(lib, "vr_set_ray_bounds")
    assert callable(getattr(capi.Context, "set_ray_bounds", None))
    assert lib.vr_set_ray_bounds(None, None, None) == capi.VR_ERR_INVALID_ARG
    for fl in ("27", "28"):
        assert re.search(r"\*\s+" + fl + r"\s+march_bound_kernel", header), fl


@pytest.mark.skipif(not os.path.exists(cer.OBJDUMP), reason="llvm-objdump of the ROCm toolchain not found")
def test_bound_kernels_in_both_units_without_scratch():
    """Exactly two code objects, the march units of namespace vr (separate multiply-adds) and of namespace vrf (fused; march_units),
    carry the 8 march_bound_kernel instances each -- BASIC (Li0) or LIGHT (Li1), 32- or 64-bit offsets, skipping or not, launches of
    one frame --, no instruction of theirs touches scratch, and the exec-region check of the two-steps-ahead kernel still passes on
    the two units."""
    regions, bad = 0, []
    for names, scratch, text in march_units("march_bound_kernel"):
        want = {f"march_bound_kernelILi{v}ELb{o32}ELb{s}ELb0EE" for v in (0, 1) for o32 in (0, 1) for s in (0, 1)}
        assert len(names) == 8 and {re.search(r"march_bound_kernelI\w+?EE", n).group(0) for n in names} == want, sorted(names)
        assert not scratch, scratch[:5]
        r, b = cer.check(text)
        regions += r
        bad += b
    assert regions >= 32 and not bad, (regions, bad[:5])


def test_bounds_bench_help():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bounds_bench.py"), "--help"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "--workload" in r.stdout, r.stderr[-2000:]
