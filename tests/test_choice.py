"""Which kernel form a march launch runs, and in what shape (csrc/vr_choice.h), on invented facts, on the CPU.

Every kernel form renders the same bits, so no frame comparison can see this code go wrong: a threshold off by one, a reroute applied
to the wrong shader or a candidate that never enters a trial only costs frame time, and a flavour that no kernel was compiled for would
leave the previous frame in the buffer.  tests/choice_driver compiles the header with g++; the cases below set the facts a launch would
have (ChoiceFacts: the request, the volumes, the tables, the machine) and the expectations are restated here from include/vr.h
(vr_set_kernel_flavour) and DESIGN 4.4, never read back from the code under test.

The sweep at the end crosses every variant, every requested flavour 0 .. 30 and a grid of facts on both sides of every threshold, and
checks that what the prior picks and every candidate has a kernel by the traits table (kShader) -- the table vr_launch.h's
`if constexpr` guards read, so there is no second list to compare it with."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(HERE, "_build")
CSRC = os.path.join(ROOT, "volumerendering_amd", "csrc")
U64 = C.c_ulonglong
M64 = (1 << 64) - 1

BASIC, LIGHT, VOLUME_MASK, THREE_FILES, MULTI_CTRT, TF_CALIB, ILLUSTRATIVE, LIGHT_INSHADER, MIP, MINIP, AVERAGE, ISO = range(12)
PLAIN, DP, PW, P2, LT, PROJ, ISOF, SHADOW, SURF, BOUND = range(10)  # KernelForm::Family


def build_driver() -> str:
    os.makedirs(OUT, exist_ok=True)
    so = os.path.join(OUT, "libchoice_driver.so")
    srcs = [os.path.join(HERE, "choice_driver", "choice_driver.cpp"), os.path.join(CSRC, "vr_choice.h"), os.path.join(CSRC, "vr_tuner.h"),
            os.path.join(ROOT, "include", "vr.h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        tmp = so + f".{os.getpid()}.tmp"
        subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Werror", "-ffp-contract=off", "-I", CSRC, "-o", tmp, srcs[0]],
                       check=True)
        os.replace(tmp, so)
    return so


class Facts(C.Structure):
    _fields_ = [("variant", C.c_int), ("rank", C.c_int), ("world", C.c_int), ("n_frames", C.c_int), ("packed", C.c_int), ("surface", C.c_int),
                ("bounded", C.c_int), ("vol", (C.c_int * 6) * 3), ("tf", (C.c_int * 5) * 2), ("layout_mode", C.c_int), ("p2_window", C.c_uint),
                ("n_cus", C.c_int), ("W", C.c_uint), ("H", C.c_uint), ("frames_in_flight", C.c_int), ("shadows", C.c_int),
                ("lights_finite", C.c_int), ("active_fraction", C.c_double), ("tuner_mode", C.c_int), ("last_chain", C.c_uint),
                ("brick_epoch", U64), ("tf_epoch", U64), ("arith", C.c_int)]


class Form(C.Structure):
    _fields_ = [("family", C.c_int), ("lanes", C.c_int), ("pipe", C.c_int), ("skip", C.c_int), ("lut", C.c_int), ("pw_threads", C.c_uint),
                ("measured", C.c_int), ("range_records", C.c_int)]


class Shape(C.Structure):
    _fields_ = [("wpb", C.c_int), ("blocks", C.c_uint), ("block", C.c_uint), ("grid", C.c_uint), ("ordered", C.c_int), ("pw", C.c_int),
                ("ltf", C.c_int), ("p2_win", C.c_int), ("lds_bytes", C.c_uint)]


class Out(C.Structure):
    _fields_ = [("p2_ok", C.c_int), ("p2_lds", C.c_uint), ("lut_ok", C.c_int), ("lut_lds", C.c_uint), ("indexable", C.c_int),
                ("can_skip", C.c_int), ("whole_frame", C.c_int), ("empty", C.c_int), ("chain_known", C.c_uint), ("prior", C.c_int),
                ("tune", C.c_int), ("n", C.c_int), ("cand", C.c_int * 6), ("shape", U64), ("key", U64)]


@pytest.fixture(scope="module")
def lib():
    L = C.CDLL(build_driver())
    L.cd_run.argtypes = [C.POINTER(Facts), C.c_int, C.POINTER(Out)]
    L.cd_form.argtypes = [C.c_int, C.c_int, C.POINTER(Form)]
    L.cd_shape.argtypes = [C.POINTER(Facts), C.c_int, C.c_int, C.c_int, C.POINTER(Shape)]
    L.cd_traits.argtypes = [C.c_int, C.POINTER(C.c_int)]
    L.cd_form_exists.argtypes = [C.c_int, C.c_int, C.c_int]
    L.cd_lights_finite.argtypes = [C.POINTER(C.c_float), C.c_int]
    L.cd_soundness.restype = U64
    L.cd_soundness.argtypes = [C.POINTER(U64), C.POINTER(C.c_int), C.POINTER(U64)]
    L.cd_bricked_slots.restype = U64
    return L


def tiles(n):
    """a viewport of n tiles of 64 x 64 pixels.  256 CUs are 256 x 4 x 5 x 64 = 327 680 hardware lanes and a tile is 4096 rays: 360 tiles
    are 4.5 rays per lane, 160 are 2.0, 96 are 1.2"""
    return dict(W=64 * n, H=64)


def facts(variant, dims=(256, 256, 256), **kw):
    """One whole frame of 360 tiles (4.5 rays per lane) on 256 CUs, one launch at a time; every volume `dims` with its bricked copy,
    density plane and brick records; both tables of 256 texels, finite, with a zero prefix; the bricked layout; finite lights; half the
    bricks active; the measured choice on; no chain known."""
    f = Facts()
    f.variant, f.rank, f.world, f.n_frames = variant, 0, 1, 1
    for i in range(3):
        f.vol[i][:] = list(kw.pop(f"dims{i}", dims)) + list(kw.pop(f"have{i}", (1, 1, 1)))
    for i in range(2):
        f.tf[i][:] = list(kw.pop(f"tf{i}", (256, 256, 3, 1, 1)))
    f.n_cus, f.frames_in_flight, f.lights_finite, f.active_fraction, f.tuner_mode = 256, 1, 1, 0.5, 1
    f.W, f.H = 64 * 360, 64
    f.brick_epoch, f.tf_epoch = 5, 9
    for k, v in kw.items():
        assert hasattr(f, k), k
        setattr(f, k, v)
    return f


def run(lib, f, requested=0):
    o = Out()
    lib.cd_run(C.byref(f), requested, C.byref(o))
    return o


def flavour(lib, f, requested=0):
    """the flavour a launch reports when nothing has been measured: what the prior picks, or what a forced flavour runs as"""
    o = run(lib, f, requested)
    if requested != 0:
        assert not o.tune and o.n == 0  # a forced flavour is never measured
    return o.prior


def cands(lib, f):
    o = run(lib, f, 0)
    assert o.tune == (o.n > 0)
    return list(o.cand)[:o.n]


# ---- the one-lane pairs -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("requested, odd", [(0, True), (1, False), (6, True), (17, True), (12, True), (30, True)])
def test_one_lane_pairs_and_their_precedence(lib, requested, odd):
    """bounded over surface over projection over ISO over shadowed LIGHT; 1 asks for the even flavour, everything else runs the odd one;
    none of them is ever measured"""
    def want(skipping):
        return skipping if odd else skipping + 1
    for v in (BASIC, LIGHT):
        assert flavour(lib, facts(v, bounded=1), requested) == want(27)
        assert flavour(lib, facts(v, surface=1), requested) == want(25)
        assert flavour(lib, facts(v, bounded=1, surface=1), requested) == want(27)
        assert flavour(lib, facts(v, bounded=1, shadows=1), requested) == want(27)
        assert flavour(lib, facts(v, surface=1, shadows=1), requested) == want(25)
    for v in (MIP, MINIP, AVERAGE):
        assert flavour(lib, facts(v), requested) == want(19)
        assert flavour(lib, facts(v, shadows=1), requested) == want(19)
        assert flavour(lib, facts(v, surface=1), requested) == want(25)  # (the order of the rows; check_render_args refuses the launch)
    assert flavour(lib, facts(ISO), requested) == want(21)
    assert flavour(lib, facts(ISO, surface=1), requested) == want(21)  # the isosurface's surface output keeps 21 / 22
    assert flavour(lib, facts(ISO, shadows=1), requested) == want(21)
    assert flavour(lib, facts(LIGHT, shadows=1), requested) == want(23)
    o = run(lib, facts(LIGHT, shadows=1), requested)
    assert not o.tune and o.n == 0
    # shadows are the lit shader's alone
    assert flavour(lib, facts(BASIC, shadows=1), requested) not in (23, 24)
    assert flavour(lib, facts(LIGHT_INSHADER, shadows=1), requested) not in (23, 24)


# ---- the prior, first part: lanes per ray from the rays per hardware lane -------------------------------------------------------
@pytest.mark.parametrize("n_tiles, kw, want", [
    (360, {}, 6), (359, {}, 11), (160, {}, 11), (159, {}, 10), (1, {}, 10),
    # chains known to be short (under 128 samples): one lane per ray from 1.2 rays per lane on
    (96, dict(last_chain=100), 6), (95, dict(last_chain=100), 10), (159, dict(last_chain=100), 6), (159, dict(last_chain=128), 6),
    (159, dict(last_chain=129), 10),
    # the rays count once per frame in flight and per frame of the launch
    (180, dict(frames_in_flight=2), 6), (179, dict(frames_in_flight=2), 11), (180, dict(n_frames=2), 6), (90, dict(n_frames=2, frames_in_flight=2), 6),
    (80, dict(n_frames=2), 11), (79, dict(n_frames=2), 10), (40, dict(n_frames=4), 11), (39, dict(n_frames=4), 10),
])
def test_first_part_thresholds(lib, n_tiles, kw, want):
    """4.5 rays per lane: one lane per ray; 2.0: two lanes (11); below: four (10); 1.2 with short chains: one.  On a shader without
    the two-steps-ahead kernel, so that the second part leaves the pick alone."""
    for tune in (0, 1):
        assert run(lib, facts(THREE_FILES, tuner_mode=tune, **tiles(n_tiles), **kw)).prior == want
    assert run(lib, facts(MULTI_CTRT, **tiles(n_tiles), **kw)).prior == want


@pytest.mark.parametrize("last_chain, short", [(0, False), (1, True), (128, True), (129, False), (4000, False)])
def test_short_chains(lib, last_chain, short):
    """last_chain is the longest chain + 1: 128 (a chain of 127) is short, 129 (128) is not, 0 is unknown.  A whole frame of the lit
    shader runs 17 unless its chains are known to be short; a forced flavour never looks the chain up."""
    o = run(lib, facts(LIGHT, last_chain=last_chain))
    assert o.chain_known == last_chain and o.prior == (6 if short else 17)
    assert run(lib, facts(LIGHT, last_chain=last_chain), 17).chain_known == 0
    assert run(lib, facts(LIGHT, last_chain=last_chain, surface=1)).chain_known == 0  # (a scene of its own)


# ---- forced flavours: what a form runs as where it cannot run --------------------------------------------------------------------
def test_persistent_forms_are_for_one_frame(lib):
    for fl in (12, 13):
        assert flavour(lib, facts(LIGHT), fl) == fl
        assert flavour(lib, facts(THREE_FILES), fl) == fl
        assert flavour(lib, facts(LIGHT, n_frames=2), fl) == 6


def test_two_steps_ahead_without_its_conditions(lib):
    no_p2 = dict(layout_mode=1)
    for v in (BASIC, LIGHT):
        assert flavour(lib, facts(v), 16) == 16 and flavour(lib, facts(v), 17) == 17
        assert flavour(lib, facts(v, n_frames=2), 16) == 16 and flavour(lib, facts(v, n_frames=2), 17) == 17
        assert flavour(lib, facts(v, **no_p2), 16) == 13 and flavour(lib, facts(v, **no_p2), 17) == 12
        assert flavour(lib, facts(v, n_frames=2, **no_p2), 16) == 6 and flavour(lib, facts(v, n_frames=3, **no_p2), 17) == 6
    # a shader without the kernel
    for v in (THREE_FILES, MULTI_CTRT, TF_CALIB, ILLUSTRATIVE):
        assert flavour(lib, facts(v), 16) == 13 and flavour(lib, facts(v), 17) == 12
        assert flavour(lib, facts(v, n_frames=2), 16) == 6 and flavour(lib, facts(v, n_frames=2), 17) == 6


def test_composite_runs_16_as_17_and_needs_its_records(lib):
    assert flavour(lib, facts(VOLUME_MASK), 16) == 17 and flavour(lib, facts(VOLUME_MASK), 17) == 17
    assert flavour(lib, facts(VOLUME_MASK, n_frames=2), 16) == 17
    for fl in (16, 17):
        for no_records in (dict(have2=(1, 1, 0)), dict(have0=(1, 1, 0)), dict(dims0=(256, 256, 252)), dict(tf0=(256, 256, -1, 1, 1))):
            assert flavour(lib, facts(VOLUME_MASK, **no_records), fl) == 12
            assert flavour(lib, facts(VOLUME_MASK, n_frames=2, **no_records), fl) == 6
    # (the lit shader's 17 runs without records as well: as the kernel that skips nothing)
    assert flavour(lib, facts(LIGHT, have0=(1, 1, 0)), 17) == 17


def test_slot_tables_in_lds(lib):
    for v in (BASIC, LIGHT, LIGHT_INSHADER):
        assert flavour(lib, facts(v), 18) == 18 and flavour(lib, facts(v, n_frames=3), 18) == 18
        assert flavour(lib, facts(v, layout_mode=1), 18) == 6
        assert flavour(lib, facts(v, have0=(0, 1, 1)), 18) == 6 and flavour(lib, facts(v, have0=(1, 0, 1)), 18) == 6
    for v in (VOLUME_MASK, THREE_FILES, MULTI_CTRT, TF_CALIB, ILLUSTRATIVE):  # the shaders that sample more than one volume
        assert flavour(lib, facts(v), 18) == 6


def test_lds_tiles_are_the_lit_shaders_one_frame(lib):
    assert flavour(lib, facts(LIGHT), 15) == 15
    assert flavour(lib, facts(LIGHT, n_frames=2), 15) == 6
    for v in (BASIC, VOLUME_MASK, THREE_FILES, MULTI_CTRT, TF_CALIB, ILLUSTRATIVE, LIGHT_INSHADER):
        assert flavour(lib, facts(v), 15) == 6


def test_illustrative_and_in_shader_gradient_reroutes(lib):
    for fl in (7, 8, 10, 11):
        assert flavour(lib, facts(ILLUSTRATIVE), fl) == 6 and flavour(lib, facts(LIGHT_INSHADER), fl) == 6
        for v in (BASIC, LIGHT, VOLUME_MASK, THREE_FILES, MULTI_CTRT, TF_CALIB):
            assert flavour(lib, facts(v), fl) == fl  # (10 / 11 of a shader without the pipelined form report 10 / 11)
    for fl in (1, 6, 12, 13):
        assert flavour(lib, facts(ILLUSTRATIVE), fl) == fl and flavour(lib, facts(LIGHT_INSHADER), fl) == fl
    # the in-shader gradient variant: the one-lane and persistent kernels only
    assert flavour(lib, facts(LIGHT_INSHADER), 16) == 13 and flavour(lib, facts(LIGHT_INSHADER), 17) == 12
    assert flavour(lib, facts(LIGHT_INSHADER, n_frames=2), 16) == 6
    # the default of either on a small launch: the first part's 10 / 11 run as 6
    for n in (359, 159, 1):
        assert run(lib, facts(ILLUSTRATIVE, **tiles(n))).prior == 6 and run(lib, facts(LIGHT_INSHADER, **tiles(n))).prior == 6


# ---- the prior, second part ------------------------------------------------------------------------------------------------------
def test_second_part_16_against_17(lib):
    for v in (BASIC, LIGHT):
        assert run(lib, facts(v, active_fraction=0.9)).prior == 16
        assert run(lib, facts(v, active_fraction=np.nextafter(0.9, 0.0))).prior == 17
        assert run(lib, facts(v, active_fraction=1.0)).prior == 16 and run(lib, facts(v, active_fraction=0.0)).prior == 17
        assert run(lib, facts(v, tf0=(256, 256, -1, 1, 1))).prior == 16  # nothing can be skipped
        # short chains: 17 gives way to the one-lane kernel, 16 (nothing to skip) does not
        assert run(lib, facts(v, last_chain=100)).prior == 6 and run(lib, facts(v, last_chain=100, active_fraction=0.95)).prior == 16
        # launches in flight and several frames per launch: the same
        assert run(lib, facts(v, frames_in_flight=2)).prior == 17 and run(lib, facts(v, n_frames=2)).prior == 17
        assert run(lib, facts(v, layout_mode=1)).prior == 6  # no bricked copy: no two-steps-ahead kernel
    # the composite: 17 whatever the share of active bricks, and only with its records
    assert run(lib, facts(VOLUME_MASK, active_fraction=0.95)).prior == 17 and run(lib, facts(VOLUME_MASK)).prior == 17
    assert run(lib, facts(VOLUME_MASK, last_chain=100)).prior == 6
    assert run(lib, facts(VOLUME_MASK, have2=(1, 1, 0))).prior == 6
    for v in (THREE_FILES, MULTI_CTRT, TF_CALIB, ILLUSTRATIVE, LIGHT_INSHADER):
        assert run(lib, facts(v)).prior == 6


def test_whole_frame_is_4_5_rays_per_lane_of_one_frame(lib):
    assert run(lib, facts(LIGHT)).whole_frame and run(lib, facts(LIGHT)).prior == 17
    o = run(lib, facts(LIGHT, **tiles(359)))
    assert not o.whole_frame and o.prior == 11
    # frames in flight fill the machine for the first part, but a share stays a share
    o = run(lib, facts(LIGHT, frames_in_flight=2, **tiles(359)))
    assert not o.whole_frame and o.prior == 6
    assert run(lib, facts(LIGHT, W=64 * 720, rank=1, world=2)).whole_frame
    assert not run(lib, facts(LIGHT, W=64 * 718, rank=1, world=2)).whole_frame
    assert run(lib, facts(LIGHT, n_cus=64, **tiles(90))).whole_frame and not run(lib, facts(LIGHT, n_cus=64, **tiles(89))).whole_frame


def test_the_prior_alone(lib):
    """tuner.mode == 0, or a share without a tile: the prior's pick, no candidates, no trial"""
    o = run(lib, facts(LIGHT, tuner_mode=0))
    assert o.prior == 17 and not o.tune and o.n == 0
    o = run(lib, facts(LIGHT, W=64, H=64, rank=1, world=2))
    assert o.empty and not o.tune and o.n == 0 and o.prior == 10
    o = run(lib, facts(LIGHT, W=64, H=64, rank=0, world=2))
    assert not o.empty and o.tune


# ---- the candidates ----------------------------------------------------------------------------------------------------------------
def test_candidate_order_and_deduplication(lib):
    """the prior's pick; 17 / 16; 6; 18; 10 / 11 (launches that leave the machine part empty) or 12 -- each once"""
    for v in (BASIC, LIGHT):
        assert cands(lib, facts(v)) == [17, 6, 18, 12]
        assert cands(lib, facts(v, active_fraction=0.95)) == [16, 6, 18, 12]
        assert cands(lib, facts(v, tf0=(256, 256, -1, 1, 1))) == [16, 6, 18, 12]
        assert cands(lib, facts(v, last_chain=100)) == [6, 17, 18, 12]
        assert cands(lib, facts(v, last_chain=100, **tiles(159))) == [6, 17, 18, 10]
        assert cands(lib, facts(v, n_frames=2)) == [17, 6, 18]  # (12 is for one frame)
        assert cands(lib, facts(v, layout_mode=1)) == [6, 12]
        assert cands(lib, facts(v, layout_mode=1, **tiles(359))) == [11, 6]
    assert cands(lib, facts(VOLUME_MASK)) == [17, 6]
    assert cands(lib, facts(VOLUME_MASK, active_fraction=0.95)) == [17, 6]
    assert cands(lib, facts(VOLUME_MASK, have2=(1, 1, 0))) == [6]
    assert cands(lib, facts(VOLUME_MASK, **tiles(159))) == [10, 17, 6]
    assert cands(lib, facts(THREE_FILES)) == [6] and cands(lib, facts(THREE_FILES, **tiles(200))) == [11, 6]
    assert cands(lib, facts(ILLUSTRATIVE)) == [6] and cands(lib, facts(ILLUSTRATIVE, **tiles(100))) == [6]
    assert cands(lib, facts(LIGHT_INSHADER)) == [6, 18] and cands(lib, facts(LIGHT_INSHADER, **tiles(100))) == [6, 18]


def test_candidate_18_needs_tables_of_8_kib_or_less(lib):
    # (nx + ny + nz + 6) * 4 bytes
    o = run(lib, facts(LIGHT, dims=(680, 680, 682)))
    assert o.lut_ok and o.lut_lds == 8192 and list(o.cand)[:o.n] == [17, 6, 18, 12]
    o = run(lib, facts(LIGHT, dims=(680, 680, 683)))
    assert o.lut_ok and o.lut_lds == 8196 and list(o.cand)[:o.n] == [17, 6, 12]
    assert flavour(lib, facts(LIGHT, dims=(680, 680, 683)), 18) == 18  # (forced, it runs up to 32 KiB)


@pytest.mark.parametrize("n_tiles, last", [(360, 12), (359, 11), (160, 11), (159, 10)])
def test_last_candidate_10_11_against_12(lib, n_tiles, last):
    for v in (BASIC, LIGHT):
        got = cands(lib, facts(v, last_chain=100, **tiles(n_tiles)))
        assert got[0] == 6 and got[-1] == last and len(got) == 4
    assert cands(lib, facts(LIGHT, n_frames=2, last_chain=100, **tiles(n_tiles)))[-1] == (18 if n_tiles >= 360 else 11 if n_tiles >= 80 else 10)
    assert cands(lib, facts(LIGHT, frames_in_flight=2, last_chain=100, **tiles(n_tiles)))[-1] == (12 if n_tiles >= 360 else 11 if n_tiles >= 80 else 10)


def test_the_trial_keys(lib):
    """shape and key as tune_pick has always been handed them"""
    def keys(f):
        shape = (0x9E3779B97F4A7C15 * ((f.variant << 56) ^ (f.world << 48) ^ (f.rank << 40) ^ (f.W << 24) ^ (f.H << 8) ^ (0x80 if f.packed else 0) ^
                                       (f.n_frames << 4) ^ f.frames_in_flight) & M64) | 1
        key = (shape ^ ((f.brick_epoch * 0xD6E8FEB86659FD93) & M64) ^ ((f.tf_epoch << 20) & M64) ^ (f.arith << 1) ^ (f.layout_mode << 2)) | 1
        return shape, key
    seen = set()
    for kw in (dict(), dict(packed=1, rank=3, world=8, W=1920, H=1080), dict(n_frames=3), dict(frames_in_flight=4), dict(arith=1),
               dict(layout_mode=3), dict(brick_epoch=(1 << 63) + 12345), dict(tf_epoch=(1 << 50) + 7)):
        for v in (BASIC, LIGHT, VOLUME_MASK):
            f = facts(v, **kw)
            o = run(lib, f)
            assert o.tune and (o.shape, o.key) == keys(f)
            seen.add((o.shape, o.key))
    assert len(seen) == 24


# ---- eligibility ---------------------------------------------------------------------------------------------------------------------
def test_p2_table_resolution(lib):
    assert run(lib, facts(LIGHT, tf0=(8190, 8190, 3, 1, 1))).p2_ok
    assert not run(lib, facts(LIGHT, tf0=(8191, 8191, 3, 1, 1))).p2_ok
    assert not run(lib, facts(LIGHT, tf0=(256, 128, 3, 1, 1))).p2_ok and not run(lib, facts(LIGHT, tf0=(128, 256, 3, 1, 1))).p2_ok
    assert run(lib, facts(LIGHT, tf1=(8191, 100, -1, 0, 0))).p2_ok  # (slot 0 alone)


def test_p2_lds_at_160_kib(lib):
    """(opacity resolution + 2) * 16 + (nx + ny + nz + 3) * 8 <= 160 KiB: a 256-texel table and nx + ny + nz = 19 961 are 163 840 bytes"""
    o = run(lib, facts(LIGHT, dims=(19953, 4, 4)))
    assert o.p2_ok and o.p2_lds == 160 * 1024
    o = run(lib, facts(LIGHT, dims=(19954, 4, 4)))
    assert not o.p2_ok and o.p2_lds == 160 * 1024 + 8
    o = run(lib, facts(LIGHT, dims=(19953, 4, 4), tf0=(257, 257, 3, 1, 1)))
    assert not o.p2_ok


def test_p2_slab_below_2_24(lib):
    """a z-slab of storage bricks (ceil(nx / 4) * ceil(ny / 4) * 64 slots) below 2^24.  With the hardware's windows (2^28 - 1 slots
    for the lit shader and the composite, 2^30 - 1 for the unlit one) such a slab fits at least 16 times: the rule "at least four
    slabs per window" can bind only under a p2_window of the tests' (next case), so window / slab of 3 against 4 has no edge to pin."""
    for v in (BASIC, LIGHT, VOLUME_MASK):
        assert not run(lib, facts(v, dims=(2048, 2048, 64))).p2_ok   # 512 * 512 * 64 = 2^24
        assert run(lib, facts(v, dims=(2048, 2044, 64))).p2_ok       # 512 * 511 * 64
        assert run(lib, facts(v, dims=(2045, 2044, 64))).p2_ok       # (bricks, not voxels)
    assert (2**28 - 1) // (512 * 511 * 64) == 16


def test_p2_window_of_the_tests(lib):
    slab = 64 * 64 * 64  # of 256^3
    for v in (BASIC, LIGHT, VOLUME_MASK):
        assert run(lib, facts(v, p2_window=3 * slab)).p2_ok
        assert not run(lib, facts(v, p2_window=3 * slab - 1)).p2_ok
        assert not run(lib, facts(v, p2_window=2 * slab)).p2_ok and run(lib, facts(v, p2_window=4 * slab)).p2_ok


def test_p2_needs_the_bricked_copy_of_the_driving_volume(lib):
    assert not run(lib, facts(LIGHT, have0=(0, 1, 1))).p2_ok and not run(lib, facts(LIGHT, have0=(1, 0, 1))).p2_ok
    assert run(lib, facts(LIGHT, have0=(1, 1, 0))).p2_ok and run(lib, facts(LIGHT, have2=(0, 0, 0), have1=(0, 0, 0))).p2_ok
    assert not run(lib, facts(LIGHT, layout_mode=1)).p2_ok and not run(lib, facts(LIGHT, layout_mode=3)).p2_ok
    # the composite's opacity is driven by volume 2
    assert not run(lib, facts(VOLUME_MASK, have2=(0, 1, 1))).p2_ok and run(lib, facts(VOLUME_MASK, have0=(0, 0, 1))).p2_ok
    # more than 2^32 slots
    assert lib.cd_bricked_slots(1624, 1624, 1632) > 1 << 32 and not run(lib, facts(LIGHT, dims=(1624, 1624, 1632))).p2_ok
    assert lib.cd_bricked_slots(1624, 1624, 1628) < 1 << 32 and run(lib, facts(LIGHT, dims=(1624, 1624, 1628))).p2_ok


def test_lut_lds_at_32_kib(lib):
    o = run(lib, facts(LIGHT, dims=(8000, 182, 4)))
    assert o.lut_ok and o.lut_lds == 32 * 1024
    o = run(lib, facts(LIGHT, dims=(8000, 183, 4)))
    assert not o.lut_ok and o.lut_lds == 32 * 1024 + 4


def test_can_skip_conditions_one_at_a_time(lib):
    for v in (BASIC, LIGHT, THREE_FILES, VOLUME_MASK, LIGHT_INSHADER):
        assert run(lib, facts(v)).can_skip and run(lib, facts(v), 6).can_skip and run(lib, facts(v), 17).can_skip
        assert not run(lib, facts(v), 1).can_skip                              # flavour 1 asks for the kernel that fetches everything
        assert not run(lib, facts(v, tf0=(256, 256, -1, 1, 1))).can_skip        # no zero prefix of the opacity table
        assert run(lib, facts(v, tf0=(256, 256, 0, 1, 1))).can_skip
        assert not run(lib, facts(v, tf0=(256, 256, 3, 0, 1))).can_skip         # colour table not finite
        assert not run(lib, facts(v, lights_finite=0)).can_skip
        assert not run(lib, facts(v, dims=(1, 8196, 16384))).can_skip           # bricks beyond the index limit
        assert run(lib, facts(v, dims=(1, 8192, 16384))).can_skip
        assert run(lib, facts(v, layout_mode=1, have0=(0, 0, 1), have2=(0, 0, 1))).can_skip  # (the records, not the bricked copy)
    for v in (MULTI_CTRT, TF_CALIB, ILLUSTRATIVE, MIP, MINIP, AVERAGE, ISO):
        assert not run(lib, facts(v)).can_skip
    for v in (BASIC, LIGHT, THREE_FILES, LIGHT_INSHADER):
        assert not run(lib, facts(v, have0=(1, 1, 0))).can_skip and run(lib, facts(v, have1=(1, 1, 0), have2=(1, 1, 0))).can_skip
    # THREE_FILES: its second table must be finite too
    assert not run(lib, facts(THREE_FILES, tf1=(256, 256, 3, 0, 1))).can_skip and not run(lib, facts(THREE_FILES, tf1=(256, 256, 3, 1, 0))).can_skip
    assert run(lib, facts(THREE_FILES, tf1=(256, 256, -1, 1, 1))).can_skip
    for v in (BASIC, LIGHT, VOLUME_MASK, LIGHT_INSHADER):
        assert run(lib, facts(v, tf1=(256, 256, 3, 0, 0))).can_skip
    # the composite: the records of volume 2 and of volume 0, on one grid
    assert not run(lib, facts(VOLUME_MASK, have2=(1, 1, 0))).can_skip and not run(lib, facts(VOLUME_MASK, have0=(1, 1, 0))).can_skip
    for a in range(3):
        d = [256, 256, 256]
        d[a] = 252
        assert not run(lib, facts(VOLUME_MASK, dims0=tuple(d))).can_skip and not run(lib, facts(VOLUME_MASK, dims2=tuple(d))).can_skip
        assert run(lib, facts(VOLUME_MASK, dims1=tuple(d))).can_skip
    assert not run(lib, facts(VOLUME_MASK, dims2=(1, 8196, 16384), dims0=(1, 8196, 16384))).can_skip
    # indexable is volume 0's
    assert run(lib, facts(LIGHT)).indexable and not run(lib, facts(LIGHT, dims0=(1, 8196, 16384))).indexable


def test_surface_launches_skip_under_the_weaker_condition(lib):
    """the brick records, a zero prefix, the index range -- the colour table and the light are not read"""
    for v in (BASIC, LIGHT):
        assert run(lib, facts(v, surface=1, tf0=(256, 256, 3, 0, 1), lights_finite=0)).can_skip
        assert not run(lib, facts(v, surface=1), 1).can_skip
        assert not run(lib, facts(v, surface=1, have0=(1, 1, 0))).can_skip
        assert not run(lib, facts(v, surface=1, tf0=(256, 256, -1, 1, 1))).can_skip
        assert not run(lib, facts(v, surface=1, dims=(1, 8196, 16384))).can_skip
    assert not run(lib, facts(ISO, surface=1)).can_skip  # (the isosurface skips by its range records)


def test_non_finite_lights_in_any_frame(lib):
    def finite(frames):
        a = np.array(frames, dtype=np.float32).reshape(-1, 12)
        return bool(lib.cd_lights_finite(a.ctypes.data_as(C.POINTER(C.c_float)), a.shape[0]))
    ok = [0.5] * 12
    assert finite([ok]) and finite([ok] * 4)
    for frame in range(4):
        for word in (0, 3, 4, 11):  # position, its fourth word, ambient, the last of diffuse
            for bad in (np.inf, -np.inf, np.nan, 2.0e15, -2.0e15):
                frames = [list(ok) for _ in range(4)]
                frames[frame][word] = bad
                assert not finite(frames), (frame, word, bad)
                assert finite(frames[:frame]) or frame == 0
    assert finite([[1.0e15] * 12, [-1.0e15] * 12])


# ---- decoding ------------------------------------------------------------------------------------------------------------------------
#        family lanes pipe skip lut threads
FORMS = {
    1: (PLAIN, 0, 0, 0, 0, 0), 6: (PLAIN, 0, 0, 0, 0, 0),
    7: (DP, 4, 0, 0, 0, 0), 8: (DP, 2, 0, 0, 0, 0), 10: (DP, 4, 1, 0, 0, 0), 11: (DP, 2, 1, 0, 0, 0),
    12: (PW, 0, 0, 0, 0, 1024), 13: (PW, 0, 1, 0, 0, 1024), 15: (LT, 0, 0, 0, 0, 0),
    16: (P2, 0, 0, 0, 0, 512), 17: (P2, 0, 0, 1, 0, 768), 18: (PLAIN, 0, 0, 0, 1, 0),
    19: (PROJ, 0, 0, 1, 0, 0), 20: (PROJ, 0, 0, 0, 0, 0), 21: (ISOF, 0, 0, 1, 0, 0), 22: (ISOF, 0, 0, 0, 0, 0),
    23: (SHADOW, 0, 0, 1, 0, 0), 24: (SHADOW, 0, 0, 0, 0, 0), 25: (SURF, 0, 0, 1, 0, 0), 26: (SURF, 0, 0, 0, 0, 0),
    27: (BOUND, 0, 0, 1, 0, 0), 28: (BOUND, 0, 0, 0, 0, 0),
}


@pytest.mark.parametrize("fl", list(range(0, 29)) + [29, 30, 99, -1])
def test_kernel_form(lib, fl):
    """every flavour 0 .. 28; the removed ones (2 .. 5, 9, 14), 0 and unknown numbers decode as the one-lane kernel"""
    for v in range(12):
        k = Form()
        lib.cd_form(fl, v, C.byref(k))
        want = list(FORMS.get(fl, (PLAIN, 0, 0, 0, 0, 0)))
        if fl == 17 and v == BASIC:
            want[5] = 1024  # (4-byte densities in the corner buffers: 4 wavefronts per SIMD)
        assert [k.family, k.lanes, k.pipe, k.skip, k.lut, k.pw_threads] == want
        assert bool(k.range_records) == (fl in (19, 20, 21, 22)) and bool(k.measured) == (not 19 <= fl <= 28)


# ---- the launch shape ----------------------------------------------------------------------------------------------------------------
def shape(lib, f, fl, off32=1, requested=None):
    s = Shape()
    lib.cd_shape(C.byref(f), fl if requested is None else requested, fl, off32, C.byref(s))
    return s


def test_shape_one_packet_per_wavefront(lib):
    """64 wavefronts per tile, one per workgroup, the tiles rounded up to 8"""
    for n, blocks in ((1, 512), (7, 512), (8, 512), (9, 1024), (360, 23040)):
        for fl in (1, 6, 18, 19, 21, 23, 25, 27, 15):
            s = shape(lib, facts(LIGHT, **tiles(n)), fl)
            assert (s.wpb, s.blocks, s.block, s.grid, s.pw) == (1, blocks, 64, blocks, 0)
    s = shape(lib, facts(LIGHT, n_frames=3, **tiles(9)), 6)
    assert (s.blocks, s.grid) == (1024, 3072)
    assert shape(lib, facts(LIGHT), 18).lds_bytes == (3 * 256 + 6) * 4 and shape(lib, facts(LIGHT), 6).lds_bytes == 0


def test_shape_depth_parallel_switches_to_four_wavefronts_per_workgroup(lib):
    """n_tiles * lanes * 64 workgroups of one wavefront up to 16 384, then a quarter as many of four"""
    for fl, lanes in ((7, 4), (10, 4), (8, 2), (11, 2)):
        edge = 16384 // (lanes * 64)
        s = shape(lib, facts(LIGHT, **tiles(edge)), fl)
        assert (s.wpb, s.blocks, s.block, s.grid) == (1, 16384, 64, 16384)
        s = shape(lib, facts(LIGHT, **tiles(edge + 1)), fl)
        assert (s.wpb, s.blocks, s.block, s.grid) == (4, (edge + 1) * lanes * 16, 256, (edge + 1) * lanes * 16)
        s = shape(lib, facts(LIGHT, **tiles(1)), fl)
        assert (s.wpb, s.blocks, s.block) == (1, lanes * 64, 64)  # (no rounding of the tiles: lanes * 64 is a multiple of 8)
        s = shape(lib, facts(LIGHT, n_frames=2, **tiles(3)), fl)
        assert (s.blocks, s.grid, s.pw, s.lds_bytes) == (3 * lanes * 64, 6 * lanes * 64, 0, 0)


def test_shape_persistent_families(lib):
    """one workgroup per CU at most, fewer when there are fewer packets; 512 / 768 / 1024 threads"""
    for fl, v, threads in ((12, LIGHT, 1024), (13, LIGHT, 1024), (12, THREE_FILES, 1024), (16, LIGHT, 512), (16, BASIC, 512), (17, LIGHT, 768),
                           (17, VOLUME_MASK, 768), (17, BASIC, 1024)):
        per = threads // 64
        for n, blocks in ((1, 512), (64, 4096), (360, 23040)):
            s = shape(lib, facts(v, **tiles(n)), fl)
            assert (s.wpb, s.blocks, s.block, s.pw) == (1, blocks, threads, 1)
            assert s.grid == min(256, -(-blocks // per))
        # the clamp at n_cus: one workgroup's worth of packets fewer than n_cus workgroups, exactly as many, one packet more
        for n_cus in (32, 31, 33, 30):
            s = shape(lib, facts(v, n_cus=n_cus, **tiles(8)), fl)
            assert s.grid == min(n_cus, -(-512 // per))
        s = shape(lib, facts(v, n_frames=1, n_cus=1000, **tiles(360)), fl)
        assert s.grid == min(1000, -(-23040 // per))
    s = shape(lib, facts(LIGHT, n_frames=2, n_cus=100, **tiles(8)), 17)  # (frame, packet) items of one queue
    assert (s.blocks, s.grid) == (512, -(-1024 // 12))
    # dynamic LDS: TF slot 0 when it fits (12, 13); TF slot 0 and the axis tables (16, 17)
    s = shape(lib, facts(LIGHT), 12)
    assert (s.ltf, s.lds_bytes, s.p2_win) == (1, 258 * 16, 0)
    s = shape(lib, facts(LIGHT, tf0=(8191, 8191, 3, 1, 1)), 12)
    assert (s.ltf, s.lds_bytes) == (0, 0)
    s = shape(lib, facts(LIGHT, tf0=(8190, 8190, 3, 1, 1)), 13)
    assert (s.ltf, s.lds_bytes) == (1, 8192 * 16)
    s = shape(lib, facts(LIGHT), 17)
    assert (s.ltf, s.lds_bytes, s.p2_win) == (1, 258 * 16 + (3 * 256 + 3) * 8, 0)
    # the moving window: a volume of 4 GiB or more, or the tests' window
    assert shape(lib, facts(LIGHT), 17, off32=0).p2_win == 1 and shape(lib, facts(LIGHT, p2_window=1 << 20), 16).p2_win == 1
    assert shape(lib, facts(LIGHT), 12, off32=0).p2_win == 0


def test_shape_ordered_up_to_196608_blocks(lib):
    assert lib.cd_order_max_blocks() == 192 * 1024
    assert shape(lib, facts(LIGHT, **tiles(3072)), 6).blocks == 196608 and shape(lib, facts(LIGHT, **tiles(3072)), 6).ordered
    s = shape(lib, facts(LIGHT, **tiles(3073)), 6)  # one group of 8 tiles more
    assert s.blocks == 196608 + 512 and not s.ordered
    # the depth-parallel kernels' blocks come in steps of lanes * 16
    assert shape(lib, facts(LIGHT, **tiles(6144)), 8).blocks == 196608 and shape(lib, facts(LIGHT, **tiles(6144)), 8).ordered
    s = shape(lib, facts(LIGHT, **tiles(6145)), 8)
    assert s.blocks == 196608 + 32 and not s.ordered
    s = shape(lib, facts(LIGHT, **tiles(3072)), 17)  # (the logical blocks, not the workgroups launched)
    assert s.ordered and s.grid == 256
    assert not shape(lib, facts(LIGHT, **tiles(3073)), 17).ordered
    assert shape(lib, facts(LIGHT, n_frames=4, **tiles(3072)), 6).ordered  # (a frame's blocks)


# ---- the table and the sweep -------------------------------------------------------------------------------------------------------
MARCH, SKIP, F_DP, DP_PIPE, F_PW, PW_PIPE, F_P2, P2_PLAIN, LUT, F_LT = (1 << i for i in range(10))
#         nvol ntf proj surface bounds skip_vol forms
TRAITS = {
    BASIC: (1, 1, 0, 1, 1, 0, MARCH | SKIP | F_DP | F_PW | PW_PIPE | F_P2 | P2_PLAIN | LUT),
    LIGHT: (1, 1, 0, 1, 1, 0, MARCH | SKIP | F_DP | DP_PIPE | F_PW | PW_PIPE | F_P2 | P2_PLAIN | LUT | F_LT),
    VOLUME_MASK: (3, 2, 0, 0, 0, 2, MARCH | SKIP | F_DP | F_PW | F_P2),
    THREE_FILES: (2, 2, 0, 0, 0, 0, MARCH | SKIP | F_DP | F_PW),
    MULTI_CTRT: (2, 2, 0, 0, 0, 0, MARCH | F_DP | F_PW),
    TF_CALIB: (2, 1, 0, 0, 0, 0, MARCH | F_DP | F_PW),
    ILLUSTRATIVE: (2, 2, 0, 0, 0, 0, MARCH | F_PW),
    LIGHT_INSHADER: (1, 1, 0, 0, 0, 0, MARCH | SKIP | F_PW | LUT),
    MIP: (1, 1, 1, 0, 0, 0, 0), MINIP: (1, 1, 1, 0, 0, 0, 0), AVERAGE: (1, 1, 1, 0, 0, 0, 0),
    ISO: (1, 1, 0, 1, 0, 0, 0),
}


def test_traits_table(lib):
    """the rows as include/vr.h describes the shaders and their forms"""
    assert lib.cd_variants() == 12
    for v, want in TRAITS.items():
        row = (C.c_int * 7)()
        lib.cd_traits(v, row)
        assert tuple(row) == want, v


def test_form_exists_follows_the_table(lib):
    for v, (_, _, proj, surface, bounds, _, forms) in TRAITS.items():
        def has(f):
            return forms & f == f
        want = {1: has(MARCH), 6: has(MARCH), 7: has(F_DP), 8: has(F_DP), 10: has(F_DP), 11: has(F_DP), 12: has(F_PW), 13: has(F_PW), 15: has(F_LT),
                16: has(P2_PLAIN), 17: has(F_P2), 18: has(MARCH | LUT), 19: bool(proj), 20: bool(proj), 21: v == ISO, 22: v == ISO,
                23: v == LIGHT, 24: v == LIGHT, 25: False, 26: False, 27: bool(bounds), 28: bool(bounds)}
        for fl, w in want.items():
            assert bool(lib.cd_form_exists(fl, v, 0)) == w, (v, fl)
        for fl in (25, 26):
            assert bool(lib.cd_form_exists(fl, v, 1)) == (bool(surface) and v != ISO), (v, fl)


def test_soundness_sweep(lib):
    """Every variant x every requested flavour 0 .. 30 x the driver's grid of facts: the flavour chosen and every candidate has a
    kernel (form_exists, after the two documented degradations: 10 / 11 and 13 of a shader without the pipelined form run without
    the pipeline); a candidate is of a measured family.

    This holds for every flavour a caller can ask for.  19 .. 28 cannot be asked for (vr_set_kernel_flavour refuses them, VR_EXP_FLAVOUR
    ignores them): they are what the one-lane families report.  choose_flavour hands such a number through as it is, so for a shader
    of another family the sweep finds no kernel behind it: counted apart, and pinned to be there, so that whoever makes them
    requestable meets this test."""
    bad, first, unsettable = U64(0), (C.c_int * 4)(), U64(0)
    n = lib.cd_soundness(C.byref(bad), first, C.byref(unsettable))
    assert bad.value == 0, (bad.value, list(first))
    assert n > 4_000_000
    assert unsettable.value > 0
    for fl in range(0, 31):
        assert bool(lib.cd_flavour_settable(fl)) == (fl in (0, 1, 6, 7, 8, 10, 11, 12, 13, 15, 16, 17, 18))
