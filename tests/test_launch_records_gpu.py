"""What feeds the measured kernel choice (flavour 0), on the device: the sort behind every march launch and the words it reports,
the span vr_kernel_times gives for real launches, and whose launches a trial's costs come from.

Every kernel form renders the same bits, so no frame comparison sees any of this go wrong.  The rules that turn these words into a
kernel are pinned on the CPU (tests/test_tuner.py); here:

* order_blocks_kernel on records made by the test, through tests/order_probe (the launch finish_slot makes: one workgroup of 1024
  threads), against a numpy restatement: a permutation inside each residue class mod 8, 128 buckets of 32 steps longest first, the
  longest chain + 1, the span, the end, the queue heads;
* vr_kernel_times of a real launch against that launch's own records, bit for bit;
* a trial's reported costs against the times of the launches in which that flavour ran, across a vr_reset_kernel_times."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import host_ref as hr
import vrtest as vt
from volumerendering_amd import build, capi

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(HERE, "_build")
CSRC = os.path.join(ROOT, "volumerendering_amd", "csrc")
f32 = np.float32
U64 = np.uint64
MAX_BLOCKS = 192 * 1024  # kOrderMaxBlocks
GUARD, HEADS = 64, 8 * 64


# ---- the sort and its reports -----------------------------------------------------------------------------------------------------
def build_probe() -> str:
    os.makedirs(OUT, exist_ok=True)
    so = os.path.join(OUT, "liborder_probe.so")
    src = os.path.join(HERE, "order_probe", "order_probe.hip")
    deps = [src] + [os.path.join(CSRC, f) for f in ("vr_frame.h", "vr_shared.h", "vr_device.h", "vr_units.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        tmp = so + f".{os.getpid()}.tmp"
        subprocess.run([build.HIPCC, *build.HIP_FLAGS, "-I", CSRC, "-o", tmp, src], check=True)
        os.replace(tmp, so)
    return so


@pytest.fixture(scope="module")
def probe():
    L = C.CDLL(build_probe())
    L.order_probe.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_ulonglong]
    assert L.order_probe_max_blocks() == MAX_BLOCKS
    return L


def run_sort(probe, rec, with_heads, with_end, heads, preset=0):
    n = rec.shape[0]
    rec = np.ascontiguousarray(rec, dtype=U64)
    order = np.full(n + GUARD, 0xFFFFFFFF, dtype=np.uint32)
    heads = heads.copy()
    words = np.zeros(3, dtype=U64)
    rc = probe.order_probe(rec.ctypes.data, n, int(with_heads), int(with_end), order.ctypes.data, heads.ctypes.data, words.ctypes.data, preset)
    assert rc == 0, rc
    return order, heads, [int(w) for w in words]


CHAINS = ["random", "equal", "zero", "rising", "falling", "one_class", "edges", "near_clamp"]
CLOCKS = ["ordinary", "high", "end_below_start"]


def make_chains(kind, n, rng):
    b = np.arange(n, dtype=np.int64)
    if kind == "random":
        return rng.integers(0, 1 << 24, n)
    if kind == "equal":
        return np.full(n, 777, dtype=np.int64)
    if kind == "zero":
        return np.zeros(n, dtype=np.int64)
    if kind == "rising":  # strictly, with the block index: every class's order is the reverse of its index order, bucket by bucket
        return b * (((1 << 24) - 1) // n)
    if kind == "falling":
        return (n - 1 - b) * (((1 << 24) - 1) // n)
    if kind == "one_class":  # class 3 holds every long chain: its buckets fill while the other classes' stay in bucket 0 / 1
        return np.where(b % 8 == 3, rng.integers(4096, 1 << 24, n), rng.integers(0, 64, n))
    if kind == "edges":  # both sides of a bucket edge (32) and of the clamp (4096 = 128 x 32)
        return rng.choice(np.array([0, 1, 31, 32, 33, 63, 64, 4031, 4032, 4063, 4064, 4095, 4096, 4097, 8191, 8192, (1 << 24) - 1]), n)
    if kind == "near_clamp":
        return rng.integers(4096 - 70, 4096 + 70, n)
    raise ValueError(kind)


def make_records(n, chains, clocks, rng):
    rec = np.zeros((n, 6), dtype=U64)
    rec[:, :3] = rng.integers(0, 1 << 40, (n, 3), dtype=np.uint64)
    if clocks == "ordinary":
        start = U64(500_000_000_000) + rng.integers(0, 1_000_000, n, dtype=np.uint64)
        end = start + rng.integers(1, 100_000, n, dtype=np.uint64)
    elif clocks == "high":
        start = U64((1 << 63) + 987_654_321) + rng.integers(0, 1_000_000, n, dtype=np.uint64)
        end = start + rng.integers(1, 100_000, n, dtype=np.uint64)
    else:  # (stale or torn records: every end lies below every start)
        start = U64(1_000_000_000) + rng.integers(0, 1_000_000, n, dtype=np.uint64)
        end = rng.integers(1000, 2000, n, dtype=np.uint64)
    rec[:, 3], rec[:, 4] = start, end
    rec[:, 5] = (chains.astype(U64) << U64(40)) | rng.integers(0, 1 << 40, n, dtype=np.uint64)  # the low 40 bits must not matter
    return rec


@pytest.mark.parametrize("n", [8, 64, 1024, 1032, 8200, MAX_BLOCKS])
def test_sort_and_reports_match_the_restatement(probe, n):
    """Fewer blocks than threads, exactly one pass, one block into the second pass, an odd number of passes (9) with a ragged last
    one, all 192 private slots; every chain pattern with every clock pattern, with and without the queue heads and the end word."""
    rng = np.random.default_rng(1000 + n)
    cls = np.arange(n) % 8
    for ci, kind in enumerate(CHAINS):
        chains = make_chains(kind, n, rng)
        assert chains.min() >= 0 and chains.max() < (1 << 24)
        bucket = np.minimum(chains >> 5, 127)
        for ki, clocks in enumerate(CLOCKS):
            with_heads, with_end = bool((ci * 3 + ki) & 1), bool((ci * 3 + ki) & 2)
            rec = make_records(n, chains, clocks, rng)
            heads_in = rng.integers(1, 1 << 32, HEADS, dtype=np.uint64).astype(np.uint32)
            preset = 0 if ki != 1 else 0xA5A5A5A5_00000000
            order, heads, (span, end, chain) = run_sort(probe, rec, with_heads, with_end, heads_in, preset)
            tag = (n, kind, clocks, with_heads, with_end)
            # the order: a permutation of 0 .. n-1 that keeps every block in its class, buckets never increasing along a class
            assert (order[n:] == 0xFFFFFFFF).all(), tag
            o = order[:n].astype(np.int64)
            assert np.array_equal(np.sort(o), np.arange(n)), tag
            assert np.array_equal(o % 8, cls), tag
            for x in range(8):
                assert (np.diff(bucket[o[x::8]]) <= 0).all(), (tag, x)
            # the words
            t0, t1 = int(rec[:, 3].min()), int(rec[:, 4].max())
            assert chain & 0xFFFFFFFF == int(chains.max()) + 1, tag
            assert span == (t1 - t0 + 1 if t1 >= t0 else 1), tag
            assert end == ((t1 | 1) if with_end else preset), tag
            # the heads: eight, 64 words apart, cleared; nothing between them touched; none without the pointer
            want = heads_in.copy()
            if with_heads:
                want[::64] = 0
            assert np.array_equal(heads, want), tag


def test_probe_refuses_what_the_context_never_launches(probe):
    rec = np.zeros((MAX_BLOCKS + 8, 6), dtype=U64)
    buf = np.zeros(MAX_BLOCKS + 8 + GUARD, dtype=np.uint32)
    for n in (0, 4, 12, MAX_BLOCKS + 8):
        assert probe.order_probe(rec.ctypes.data, n, 0, 0, buf.ctypes.data, buf.ctypes.data, rec.ctypes.data, 0) == -1


# ---- the span of real launches ----------------------------------------------------------------------------------------------------
def lit_scene(ctx, n, W, H, **kw):
    vols, tfs = vt.scene(capi.LIGHT, n=n)
    step, count = hr.stepping_params(n, n, n)
    u = hr.make_uniforms(W, H, steps_count=count, step_size=step, **kw)
    for i, v in enumerate(vols):
        ctx.volume_upload(i, v)
    for i, t in enumerate(tfs):
        ctx.tf_upload(i, t[0], t[1])
    ctx.set_uniforms(vt.to_capi_uniforms(u))


def test_kernel_time_is_the_span_of_the_launch_s_own_records():
    """Forced flavours 6, 11, 10, 12 and 17 (one packet per workgroup, two and four lanes per ray, persistent wavefronts without and
    with the pipeline: the last two index their records by logical block): after every synchronous render vr_kernel_times' newest
    value is float32((max(end) - min(start)) x 1e-5) of that launch's records, bit for bit; no record ends before it starts; the
    records' sums are the counters.

    A launch without a sort behind it is timed with HIP events, and only a positive time can be asked of it.  The launch shapes make
    every block count a multiple of eight (whole groups of eight tiles of 64 packets; 128 or 256 workgroups per tile in the
    depth-parallel forms), so no viewport gives a launch that is left unsorted for its count's residue: the launches timed with
    events are the ones above kOrderMaxBlocks blocks and the ones vr_set_kernel_timing asks for, and both are run here."""
    W, H = 200, 120
    with capi.Context(W, H, 0) as ctx:
        lit_scene(ctx, 32, W, H)
        for rnd in range(2):
            for fl, blocks in ((6, 512), (11, 1024), (10, 2048), (12, 512), (17, 512)):
                ctx.set_kernel_flavour(fl)
                ctx.render(capi.LIGHT)
                assert ctx.last_kernel_flavour() == fl
                t = ctx.kernel_times(1)
                rec = ctx.block_trace().astype(U64)
                assert rec.shape == (blocks, 6) and blocks % 8 == 0, (fl, rec.shape)
                start, end = rec[:, 3], rec[:, 4]
                assert (start <= end).all(), fl
                want = f32(np.float64(int(end.max()) - int(start.min())) * 1.0e-5)
                assert t.shape == (1,) and t[0].tobytes() == want.tobytes(), (fl, t, want)
                assert t[0] > 0.0
                assert tuple(int(rec[:, i].sum()) for i in range(3)) == tuple(ctx.counters()), fl
        # timed with events because the caller says so: a positive time, and the records' span is not what is reported
        ctx.set_kernel_timing(True)
        ctx.set_kernel_flavour(6)
        ctx.render(capi.LIGHT)
        t = ctx.kernel_times(1)
        assert t.shape == (1,) and t[0] > 0.0
        ctx.set_kernel_timing(False)
    # ... and because the launch has more blocks than the sort takes
    W, H = 4096, 3136
    with capi.Context(W, H, 0) as ctx:
        lit_scene(ctx, 32, W, H)
        ctx.set_kernel_flavour(6)
        ctx.render(capi.LIGHT)
        n_blocks = ctx.block_trace().shape[0]
        assert n_blocks == (W // 64) * (H // 64) * 64 and n_blocks > MAX_BLOCKS
        t = ctx.kernel_times(1)
        assert t.shape == (1,) and t[0] > 0.0


# ---- whose launches a trial's costs come from ---------------------------------------------------------------------------------------
def test_trial_costs_are_the_times_of_that_flavour_s_own_launches_across_a_reset():
    """The scene of test_measured_kernel_choice_settles_and_changes_nothing, one synchronous flavour-0 render at a time, with the
    flavour that ran and vr_kernel_times' newest value noted after each, and ONE vr_reset_kernel_times in the middle of the trial:
    right behind the first candidate's last trial launch (four settling launches, three of its turn: the seventh render), as
    bench.py's reset between warm-up and timed frames may fall.  The reset empties what vr_kernel_times reports, so a step's time is
    read before that step's reset.

    Frames stay flavour 6's; a choice is made; every candidate's reported cost is, to within two ticks (the tuner keeps the raw
    span + 1), the time noted for one of the launches in which that flavour ran.  A trial that named its launches by a counter the
    reset rewinds reads the first candidate's cost from the later candidates' launches."""
    n, W, H = 48, 640, 400
    vols, tfs = vt.scene(capi.LIGHT, n=n)
    step, count = hr.stepping_params(n, n, n)
    u = hr.make_uniforms(W, H, steps_count=count, step_size=step, distance=1.0)
    with capi.Context(W, H, 0) as ctx:
        ctx.set_kernel_flavour(6)
        ref, _, n_ref = vt.gpu_render(ctx, capi.LIGHT, u, vols, tfs)
        ctx.set_kernel_flavour(0)
        ran, times = [], []
        chosen = -1
        for k in range(60):
            ctx.render(capi.LIGHT)
            frag, _, ns = ctx.download()
            assert ns == n_ref and np.array_equal(vt.bits(frag), vt.bits(ref)), k
            ran.append(ctx.last_kernel_flavour())
            t = ctx.kernel_times(1)
            assert t.shape == (1,) and t[0] > 0.0, k
            times.append(float(t[0]))
            if k == 4 + 3 - 1:
                ctx.reset_kernel_times()
                assert ctx.kernel_times(1).shape == (0,)
            cands, ms, chosen = ctx.kernel_choice()
            if chosen >= 0 and k >= 4 + 3 * len(cands) + 4:
                break
        assert chosen >= 0 and len(cands) >= 2, (cands, ms, chosen, ran)
        assert ran[:7] == [cands[0]] * 7 and ran[7:10] == [cands[1]] * 3, (ran, cands)  # (the reset fell where it was meant to)
        assert ran[-1] == cands[chosen]
        print("ran", ran, "\ntimes", times, "\ncands", cands, "ms", list(ms), "chosen", chosen)
        for f, cost in zip(cands, ms):
            own = np.array([t for g, t in zip(ran, times) if g == f])
            assert own.size >= 3 and np.abs(own - float(cost)).min() <= 2.0e-5, (f, float(cost), own, cands, list(ms))


def test_a_share_without_a_tile_opens_no_trial():
    """A rank whose share of the tiles is empty launches nothing and takes no launch number, so the measured choice is not consulted
    for it: a trial that counted such calls would hold one launch number many times over (and take one of the eight slots for a
    shape that never renders).  The rank that does hold the tile gets its trial, and its costs are its own launches' times."""
    W, H = 64, 64
    with capi.Context(W, H, 0) as ctx:
        lit_scene(ctx, 24, W, H, distance=1.0)
        ctx.set_kernel_flavour(0)
        assert ctx.tile_count(1, 2) == 0 and ctx.tile_count(0, 2) == 1
        for _ in range(20):
            ctx.render_tiles(capi.LIGHT, 1, 2)
        assert ctx.kernel_choice() == ([], [], -1)
        assert ctx.kernel_times(8).shape == (0,)
        ran, times = [], []
        for k in range(40):
            ctx.render_tiles(capi.LIGHT, 0, 2)
            ran.append(ctx.last_kernel_flavour())
            times.append(float(ctx.kernel_times(1)[0]))
            ctx.render_tiles(capi.LIGHT, 1, 2)  # (in between: nothing)
            assert ctx.kernel_times(1)[0] == f32(times[-1])
        cands, ms, chosen = ctx.kernel_choice()
        assert chosen >= 0 and len(cands) >= 2, (cands, ms, chosen, ran)
        for f, cost in zip(cands, ms):
            own = np.array([t for g, t in zip(ran, times) if g == f])
            assert own.size >= 3 and np.abs(own - float(cost)).min() <= 2.0e-5, (f, float(cost), own)
