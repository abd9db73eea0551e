"""CPU side of the random feature sweep: on the seeded cases of feature_cases.py (non-cubic volumes, ragged viewports, random cameras,
clips, stepping and tables) every float32 restatement the GPU sweep compares against -- proj_ref, bound_ref, surf_ref, shadow_ref,
iso_ref -- is pinned to the oracle wherever include/vr.h makes the two identical, bit for bit and with the counters, once in
separately rounded arithmetic and once more with fused=True against the oracle's fused mode; per family at least two cases in three
are ones where the feature acts (judged on the restatements alone, in either mode), so that the GPU sweep over the same cases
compares frames that have something in them; and per family the fused restatement differs from the separate one in at least one
such case, so that fused=True is known to do something."""
import functools

import numpy as np
import pytest

import bound_ref as br
import feature_cases as fc
import iso_ref as ir
import oracle_binding as ob
import proj_ref as pr
import shadow_ref as shr
import surf_ref as sr
import vrtest as vt

f32 = np.float32


def same(a, b):
    """Bit-equal, NaN where the other is NaN."""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    fin = ~np.isnan(b)
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(vt.bits(a)[fin], vt.bits(b)[fin])


def iso_pins(c, u, what, fused=False):
    """ISO on a seeded subset of rays against the positions surf_ref places and the densities proj_ref's sampler reads there: the hit
    is the first in-box step at or above the level, its position is that step's, composited counts the in-box steps up to it (all of
    them without a hit: MIP's count), and the refined point lies between the hit step and the one before it."""
    rng = np.random.default_rng(c.seed * 1000 + c.index)
    pix = np.stack([rng.integers(0, c.W, 300), rng.integers(0, c.H, 300)], 1)
    r = ir.march(u, c.W, c.H, c.vec4, c.tf, c.iso, pixels=pix, fused=fused)
    s = sr.march(u, c.W, c.H, c.vec4, c.tf[0], 0.5, pixels=pix, positions=True, fused=fused)
    _, n_mip, _, _ = pr.march(pr.MIP, u, c.W, c.H, c.vec4, c.tf, pixels=pix, fused=fused)
    assert np.array_equal(r["hit"], r["covered"]) and not np.any(r["hit"] & ~s["rayhit"]), what
    if u.steps_count <= 0 or not s["rayhit"].any():
        assert not r["hit"].any() and not r["composited"].any(), what
        return
    P = s["positions"]  # (steps, N, 3)
    lo, hi = shr.clip_box(u)
    with np.errstate(all="ignore"):
        inb = np.all((P >= lo) & (P <= hi), axis=2)
    dens = np.ascontiguousarray(c.vec4[..., 3])
    d = pr.sample_a(dens, P.reshape(-1, 3), fused).reshape(P.shape[:2])
    above = inb & (d >= f32(c.iso))
    hit = above.any(axis=0)
    k = np.argmax(above, axis=0)
    counted = np.where(hit, np.take_along_axis(np.cumsum(inb, axis=0), k[None], 0)[0], inb.sum(axis=0))
    assert np.array_equal(r["hit"], hit), what
    assert np.array_equal(r["composited"], counted), what
    assert np.array_equal(r["composited"][~hit], n_mip[~hit]) and np.all(r["composited"] <= n_mip), what
    h = np.nonzero(hit)[0]
    pk = P[k[h], h]
    assert np.array_equal(vt.bits(r["pk"][h]), vt.bits(pk)), what
    prev = P[np.maximum(k[h] - 1, 0), h]
    q = r["q"][h]
    between = np.all((q >= np.minimum(prev, pk)) & (q <= np.maximum(prev, pk)), axis=1)
    assert np.all(between), what
    assert np.all(r["frag"][hit, 3] == f32(1.0)) and not np.any(r["frag"][~hit]), what


MODES = ((False, ob.SEPARATE), (True, ob.FUSED))  # (the restatements' fused=, the oracle's arithmetic)


@functools.lru_cache(maxsize=None)
def sweep(seed):
    """Every pin on every case of a seed, in both arithmetic modes; returns ({fused: {family: cases where the feature acts}}, {family:
    cases where it acts and the fused restatement's frame or counters differ from the separate one's}) (computed once per session)."""
    acts = {fused: {f: 0 for f in fc.FAMILIES} for fused, _ in MODES}
    differs = {f: 0 for f in fc.FAMILIES}
    for c in fc.cases(seed):
        u = c.uniforms()
        W, H, v, tf = c.W, c.H, c.vec4, c.tf
        refs = {}
        for fused, oracle_mode in MODES:
            what = (seed, c.index, "fused" if fused else "separate", c.draw)
            with ob.arithmetic(oracle_mode):
                plain = {var: ob.render(var, u, [v], [tf], W, H, nthreads=8) for var in (fc.BASIC, fc.LIGHT)}
                flat = fc.flat_tf(c.tf_res)
                first, n_first, _ = ob.render(fc.LIGHT, u, [v], [flat], W, H, nthreads=8)

            def is_plain(got, var):
                return same(got[0], plain[var][0]) and tuple(got[1:]) == tuple(plain[var][1:])

            # BASIC through the projections' march
            assert is_plain(pr.frame(pr.BASIC, u, W, H, v, tf, fused=fused), fc.BASIC), ("proj_ref BASIC", what)
            # no bounds, and bounds that cut nothing
            free = {var: br.frame(var, u, W, H, v, tf, fused=fused) for var in (fc.BASIC, fc.LIGHT)}
            for var in (fc.BASIC, fc.LIGHT):
                assert is_plain(free[var], var), ("bound_ref without bounds", var, what)
            var = c.bound_variant
            zero, one = np.zeros((H, W), f32), np.ones((H, W), f32)
            assert is_plain(br.frame(var, u, W, H, v, tf, zero, one, fused=fused), var), ("bound_ref near 0 far 1", var, what)
            # the alpha plane of the surface output at the shaders' own cut-offs
            for var, tau in ((fc.BASIC, sr.TAU_BASIC), (fc.LIGHT, sr.TAU_LIGHT)):
                s, n_s, hits = sr.frame(u, W, H, v, tf[0], tau, fused=fused)
                assert same(s[..., 3], plain[var][0][..., 3]), ("surf_ref alpha", var, what)
                assert n_s == plain[var][1] and hits == int((plain[var][0][..., 3] > tau).sum()), ("surf_ref counts", var, what)
            # shadows off, and a light volume that shadows nothing
            assert is_plain(shr.frame(u, W, H, v, tf, None, fused=fused), fc.LIGHT), ("shadow_ref without a light volume", what)
            grid = fc.light_volume(c, u, scale=0.0, fused=fused)
            assert grid.shape == shr.grid_of(v.shape, c.shadow_divisor)[::-1] and np.all(grid == f32(1.0)), ("shadow_ref.build at scale 0", what)
            assert is_plain(shr.frame(u, W, H, v, tf, grid, fused=fused), fc.LIGHT), ("shadow_ref at scale 0", what)
            # the isosurface: a level below every sample under an opaque constant table is LIGHT's first sample; the hit logic
            got, n, _ = ir.frame(u, W, H, v, flat, -1.0, fused=fused)
            assert same(got, first) and n == n_first, ("iso_ref at the first sample", what)
            iso_pins(c, u, ("iso_ref hit", what), fused)
            # where the features act
            for fam in fc.FAMILIES:
                if fam != "bound":
                    refs[fused, fam] = fc.reference(c, fam, u, fused=fused)
                else:  # (fc.reference's frame, with what the march says about the bounds)
                    placed = br.march(c.bound_variant, u, W, H, v, tf, c.near, c.far, fused=fused)
                    refs[fused, "placement"] = [placed[k] for k in ("before_far", "before_near", "prefix")]
                    refs[fused, fam] = placed["frag"].reshape(H, W, 4), int(placed["composited"].sum()), int(placed["covered"].sum())
                refs[fused, fam, "acts"] = bool(fc.acts(c, fam, refs[fused, fam], free))
                acts[fused][fam] += refs[fused, fam, "acts"]
        # sigma, g(d), S_near / S_far are ray placement: which steps lie before a bound is the same in both modes, ties included
        for a, b in zip(refs[False, "placement"], refs[True, "placement"]):
            assert np.array_equal(a, b), ("bound_ref: the bounds cut other steps in fused mode", seed, c.index, c.draw)
        for fam in fc.FAMILIES:
            (fs, ns, cs), (ff, nf, cf) = refs[False, fam], refs[True, fam]
            differs[fam] += bool(refs[False, fam, "acts"] and refs[True, fam, "acts"] and not (same(ff, fs) and (nf, cf) == (ns, cs)))
    for fused, _ in MODES:
        print("fused" if fused else "separate", "feature acts in", acts[fused], "of", fc.CASES_PER_SEED, "cases of seed", seed)
    print("the fused restatement differs from the separate one in", differs, "of them")
    return acts, differs


@pytest.mark.parametrize("seed", fc.SEEDS)
def test_restatements_pin_to_the_oracle(seed):
    sweep(seed)


def test_two_cases_in_three_are_non_trivial():
    """Per family, over all seeds: the feature acts (composited > 0; ISO / surface: a hit; bounds: fewer composited samples than the
    unbounded frame; shadows at a scale above 0: not LIGHT's frame) in at least two thirds of the cases, in the separately rounded
    restatements and in the fused ones alike."""
    total = len(fc.SEEDS) * fc.CASES_PER_SEED
    for fused, _ in MODES:
        counts = {f: sum(sweep(s)[0][fused][f] for s in fc.SEEDS) for f in fc.FAMILIES}
        print("fused" if fused else "separate", "non-trivial cases per family:", counts, "of", total)
        for f, n in counts.items():
            assert 3 * n >= 2 * total, (f, fused, n, total)


def test_the_fused_switch_does_something():
    """Per family, over all seeds: in at least one case where the feature acts the fused restatement's frame differs in at least one
    bit (or a counter) from the separate restatement's -- fused=True reaches the family's arithmetic."""
    counts = {f: sum(sweep(s)[1][f] for s in fc.SEEDS) for f in fc.FAMILIES}
    print("cases whose fused restatement differs from the separate one, per family:", counts)
    for f, n in counts.items():
        assert n >= 1, (f, n)
