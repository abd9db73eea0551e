"""The rules of the measured kernel choice (flavour 0; csrc/vr_tuner.h: tune_pick) on invented launch records, on the CPU.

Every kernel form renders the same bits, so no frame comparison can see this code go wrong: a margin applied to the wrong
candidate or a cost read from another launch's slot only costs frame time.  tests/tuner_driver compiles the header with g++
behind a model of the context's kernel-time ring; the scripts below say which launch reports which span and end, and when, and
the expectations are restated here from the rules (include/vr.h, vr_set_kernel_flavour), never read back from the
tuner.  A launch is `pick` (what choose_flavour asks) followed by `launch` (the number it takes, its slot zeroed); its report
arrives `lag` launches later, as a sort's does with frames in flight.

A pick that no launch follows would leave two entries of a trial naming one launch number.  tune_pick cannot know, so the rule is
its caller's: enqueue_render's branch without a kernel (a rank's share without a tile) takes no launch number, and
choose_flavour therefore never consults the tuner for it (tests/test_launch_records_gpu.py pins that on the device;
test_every_trial_launch_has_a_number_of_its_own pins the invariant here).  A pick's own launch (vr_pick) is a surface launch,
which is never measured and never reaches tune_pick."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(HERE, "_build")
CSRC = os.path.join(ROOT, "volumerendering_amd", "csrc")
f32 = np.float32
U64 = C.c_ulonglong


def build_driver() -> str:
    os.makedirs(OUT, exist_ok=True)
    so = os.path.join(OUT, "libtuner_driver.so")
    srcs = [os.path.join(HERE, "tuner_driver", "tuner_driver.cpp"), os.path.join(CSRC, "vr_tuner.h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        tmp = so + f".{os.getpid()}.tmp"
        subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Werror", "-ffp-contract=off", "-I", CSRC, "-o", tmp, srcs[0]],
                       check=True)
        os.replace(tmp, so)
    return so


@pytest.fixture(scope="module")
def lib():
    L = C.CDLL(build_driver())
    L.td_create.restype = C.c_void_p
    L.td_create.argtypes = [C.c_int]
    L.td_destroy.argtypes = [C.c_void_p]
    L.td_pick.argtypes = [C.c_void_p, U64, U64, C.POINTER(C.c_int), C.c_int, C.c_uint, C.c_int, C.c_int]
    L.td_launch.restype = C.c_longlong
    L.td_launch.argtypes = [C.c_void_p]
    L.td_report.argtypes = [C.c_void_p, C.c_longlong, U64, U64]
    L.td_reset.argtypes = [C.c_void_p]
    L.td_head.restype = C.c_longlong
    L.td_head.argtypes = [C.c_void_p]
    L.td_reported.restype = C.c_longlong
    L.td_reported.argtypes = [C.c_void_p]
    L.td_choice.argtypes = [C.c_void_p, U64, C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_int)]
    L.td_launches.argtypes = [C.c_void_p, U64, C.POINTER(C.c_longlong), C.POINTER(C.c_uint)]
    L.td_slots.argtypes = [C.c_void_p, C.POINTER(U64)]
    L.td_latest.restype = U64
    L.td_latest.argtypes = [C.c_void_p]
    return L


def per_of(in_flight):
    return 3 if in_flight == 1 else 3 * in_flight + 2


def settle_of(in_flight):
    return in_flight + 3


def ms(ticks):
    """a cost as reported: 100 MHz ticks -> ms, in double, then float32"""
    return f32(np.float64(ticks) * 1.0e-5)


class Sim:
    """One context's launches.  `log` holds (flavour, launch number, span, end, key) of every launch made through frame()."""

    def __init__(self, lib, rewind=False):
        self.lib, self.h = lib, lib.td_create(int(rewind))
        self.step, self.origin, self.pending, self.log = 0, 0, [], []

    def close(self):
        self.lib.td_destroy(self.h)

    def pick(self, key, cand, shape=1, chain=0, measurable=True, in_flight=1):
        arr = (C.c_int * len(cand))(*cand)
        return self.lib.td_pick(self.h, key, shape, arr, len(cand), chain, int(measurable), in_flight)

    def launch(self, span, end, lag=0):
        """takes the next launch number; the report (span, end; span None: never) arrives after `lag` more launches"""
        L = self.lib.td_launch(self.h)
        if span is not None:
            self.pending.append((self.step + lag, L, span, end))
        self.step += 1
        due = [p for p in self.pending if p[0] < self.step]
        self.pending = [p for p in self.pending if p[0] >= self.step]
        for _, l, s, e in due:
            self.lib.td_report(self.h, l, s, e)
        return L

    def mark(self):
        """a new script starts here: records() counts its steps from this launch on"""
        self.origin = self.step

    def frame(self, key, cand, records, lag=0, **kw):
        """pick + launch; records(flavour, step of the script) -> (span, end)"""
        f = self.pick(key, cand, **kw)
        span, end = records(f, self.step - self.origin)
        L = self.launch(span, end, lag)
        self.log.append((f, L, span, end, key))
        return f

    def head(self):
        return self.lib.td_head(self.h)

    def reset(self):
        self.lib.td_reset(self.h)

    def choice(self, key):
        cand, cost, ch = (C.c_int * 6)(), (C.c_float * 6)(), C.c_int(-9)
        n = self.lib.td_choice(self.h, key, cand, cost, C.byref(ch))
        if n < 0:
            return None
        return list(cand)[:n], np.array(list(cost)[:n], dtype=f32), ch.value

    def launches(self, key):
        buf, ref = (C.c_longlong * 96)(), C.c_uint(0)
        per = self.lib.td_launches(self.h, key, buf, C.byref(ref))
        return np.array(list(buf), dtype=np.int64).reshape(6, 16), per, ref.value

    def slots(self):
        keys = (U64 * 8)()
        self.lib.td_slots(self.h, keys)
        return list(keys)


@pytest.fixture
def sim(lib):
    s = Sim(lib)
    yield s
    s.close()


CANDS = [17, 6, 18, 12, 16, 10]


def one_at_a_time(costs):
    """records of launches one at a time: flavour f's spans are costs[f] + 7 and costs[f], its FIRST trial launch (and whatever it
    runs while settling or waiting) far below both: a cost that counted a first launch would show"""
    def records(f, step):
        k = step - settle_of(1)
        q = k % 3 if k >= 0 else 0
        return (costs[f] - 500 if q == 0 else costs[f] + (7 if q == 1 else 0)), 1
    return records


class Clock:
    """records of launches in flight: every launch of flavour f ends costs[f] ticks after the launch before it (the span says nothing)"""

    def __init__(self, costs, wobble=None):
        self.costs, self.now, self.wobble = costs, 1000001, wobble or (lambda step: 0)

    def __call__(self, f, step):
        self.now += self.costs[f] + 2 * self.wobble(step)
        return 12345, self.now


def decide(sim, cand, costs, in_flight=1, key=11, shape=1, chain=0, extra=6):
    """a whole trial of `cand` with the given cost per candidate (ticks): the flavours that ran, and what was decided"""
    by_f = dict(zip(cand, costs))
    records = one_at_a_time(by_f) if in_flight == 1 else Clock(by_f)
    lag = 0 if in_flight == 1 else in_flight
    n = settle_of(in_flight) + len(cand) * per_of(in_flight) + lag + extra
    sim.mark()
    ran = [sim.frame(key, cand, records, lag=lag, in_flight=in_flight, shape=shape, chain=chain) for _ in range(n)]
    return ran, sim.choice(key)


def kept(costs, in_flight):
    """the margin rule on reported costs (float32): index of the candidate that stays"""
    best = 0
    for i in range(1, len(costs)):
        bar = costs[best] * f32(0.95 if in_flight > 1 else 0.98) if best == 0 else costs[best]
        if costs[i] < bar:
            best = i
    return best


def schedule(cand, in_flight, lag=0):
    """what runs until the choice: settling, the turns in candidate order, the first candidate while the last reports are out"""
    out = [cand[0]] * settle_of(in_flight)
    for f in cand:
        out += [f] * per_of(in_flight)
    return out + [cand[0]] * lag


# ---- one candidate, settling, turns, waiting --------------------------------------------------------------------------------------
def test_one_candidate_is_returned_at_once_and_takes_no_slot(sim):
    for _ in range(5):
        assert sim.frame(5, [12], one_at_a_time({12: 1000})) == 12
    assert sim.slots() == [0] * 8 and sim.choice(5) is None and sim.lib.td_latest(sim.h) == 0


@pytest.mark.parametrize("in_flight", [1, 2, 3, 4])
def test_settling_turns_and_waiting(sim, in_flight):
    """in_flight + 3 launches of the first candidate, then `per` launches of each in candidate order (3, or 3 x in_flight + 2), then
    the first candidate again until the last report is in; the call after that makes the choice, once."""
    cand = CANDS[:4]
    costs = dict(zip(cand, [50000, 40000, 30000, 45000]))
    lag = in_flight + 1
    records = Clock(costs) if in_flight > 1 else one_at_a_time(costs)
    want = schedule(cand, in_flight, lag)
    for k, f in enumerate(want):
        assert sim.choice(7) is None or sim.choice(7)[2] == -1, k
        assert sim.frame(7, cand, records, lag=lag, in_flight=in_flight) == f, k
    assert sim.choice(7)[2] == -1
    launches, per, _ = sim.launches(7)
    assert per == per_of(in_flight)
    first = settle_of(in_flight)
    assert np.array_equal(launches[:4, :per].ravel(), np.arange(first, first + 4 * per))  # every trial launch, in order, once
    assert (launches[4:] == -1).all() and (launches[:4, per:] == -1).all()
    assert sim.frame(7, cand, records, lag=lag, in_flight=in_flight) == 18
    got, cost, chosen = sim.choice(7)
    assert got == cand and chosen == 2
    # ... once: the records of later launches (they overwrite nothing of the trial's here, but they are new) change nothing
    slow = {f: c // 10 if f == 17 else 10 * c for f, c in costs.items()}
    slow = Clock(slow) if in_flight > 1 else one_at_a_time(slow)
    for _ in range(3 * per):
        assert sim.frame(7, cand, slow, lag=lag, in_flight=in_flight) == 18
    assert np.array_equal(sim.choice(7)[1], cost) and sim.choice(7)[2] == 2


def test_every_trial_launch_has_a_number_of_its_own(sim):
    """(see the module's docstring: a pick that no launch follows is the caller's to avoid)  With a launch behind every pick the
    numbers a trial holds are distinct, whatever else runs in between; a pick without a launch is what breaks it."""
    cand = CANDS[:3]
    rec = one_at_a_time(dict(zip(cand, [900, 800, 700])))
    for k in range(4 + 9):
        sim.frame(3, cand, rec)
        sim.launch(55, 1)  # somebody else's launch
    launches, per, _ = sim.launches(3)
    held = launches[:3, :per].ravel()
    assert len(set(held)) == 9 and (held >= 0).all()
    other = Sim(sim.lib)
    try:
        for k in range(4 + 9):
            other.pick(3, cand)  # (no launch: the counter stands still)
        held = other.launches(3)[0][:3, :3].ravel()
        assert len(set(held)) == 1
    finally:
        other.close()


def test_unmeasurable_launches_run_the_first_candidate_and_settle_nothing(sim):
    cand = CANDS[:2]
    rec = one_at_a_time({17: 5000, 6: 4000})
    for _ in range(9):
        assert sim.frame(9, cand, rec, measurable=False) == 17
    assert sim.choice(9)[2] == -1 and (sim.launches(9)[0] == -1).all()
    ran = [sim.frame(9, cand, rec) for _ in range(4 + 6 + 1)]
    assert ran == schedule(cand, 1) + [6]


# ---- costs -------------------------------------------------------------------------------------------------------------------------
def test_cost_one_at_a_time_is_the_smallest_span_but_the_first(sim):
    cand = CANDS[:3]
    spans = {}

    def records(f, step):
        spans[step] = 70000 + 1000 * cand.index(f) + [0, 900, 40, 650, 5, 333, 77, 0, 800, 900, 3, 950, 20, 1][step]
        return spans[step], 1
    ran = [sim.frame(2, cand, records) for _ in range(4 + 9 + 1)]
    assert ran[:-1] == schedule(cand, 1)
    got, cost, chosen = sim.choice(2)
    want = [ms(min(spans[4 + 3 * i + 1], spans[4 + 3 * i + 2])) for i in range(3)]
    assert got == cand and [c.tobytes() for c in cost] == [w.tobytes() for w in want]  # in ms, in candidate order, bit for bit
    # (17: 70000 + min(333, 77), not its first launch's 5; 6: 71800, not the first's 71000; 18: 72020, not 72003)
    assert [float(w) for w in want] == [float(ms(70077)), float(ms(71800)), float(ms(72020))]
    assert chosen == 0 and ran[-1] == 17  # neither is below 0.98 x 70077


@pytest.mark.parametrize("in_flight", [2, 3, 4])
def test_cost_in_flight_is_the_mean_interval_of_the_interior_ends(sim, in_flight):
    cand = CANDS[:3]
    f, per = in_flight, per_of(in_flight)
    records = Clock(dict(zip(cand, [60000, 50000, 64000])), wobble=lambda step: (step * 7919) % 1013)
    n = settle_of(f) + 3 * per + f
    ran = [sim.frame(4, cand, records, lag=f, in_flight=f) for _ in range(n + 1)]
    assert ran[:-1] == schedule(cand, f, f)
    got, cost, chosen = sim.choice(4)
    want = []
    for i in range(3):
        ends = [e for (_, _, _, e, _) in sim.log[settle_of(f) + i * per:settle_of(f) + (i + 1) * per]]
        want.append(ms((ends[per - f] - ends[f]) / np.float64(per - 2 * f)))
    assert [c.tobytes() for c in cost] == [w.tobytes() for w in want]
    assert chosen == 1 and ran[-1] == 6


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("backwards", [0, 1])
def test_ends_that_do_not_advance_are_unusable(sim, which, backwards):
    """e1 <= e0 (equal, or a clock that went backwards): that candidate's cost is 1e18 ticks -- a challenger never wins with it,
    a prior with it loses to any challenger."""
    cand = CANDS[:2]
    f, per = 2, 8
    first = settle_of(f) + which * per

    def records(fl, step):
        e = 5000001 + 30000 * step
        if step == first + per - f:
            e = 5000001 + 30000 * (first + f) - 2 * backwards
        return 1, e
    ran = [sim.frame(6, cand, records, lag=f, in_flight=f) for _ in range(settle_of(f) + 2 * per + f + 1)]
    _, cost, chosen = sim.choice(6)
    assert cost[which].tobytes() == f32(1.0e18 * 1.0e-5).tobytes() and cost[1 - which].tobytes() == ms(30000).tobytes()
    assert chosen == 1 - which and ran[-1] == cand[1 - which]


# ---- the margin --------------------------------------------------------------------------------------------------------------------
PRIOR = 100000


@pytest.mark.parametrize("in_flight, costs, keeps", [
    (1, [PRIOR, 97900], 1), (1, [PRIOR, 98100], 0), (1, [PRIOR, 98000 + 2], 0),
    (3, [PRIOR, 94900], 1), (3, [PRIOR, 95100], 0), (3, [PRIOR, 97900], 0),
    # between challengers strictly smaller wins: a third that beats the second by less than 2 % (5 %) replaces it, an equal one does not
    (1, [PRIOR, 90000, 89000], 2), (1, [PRIOR, 90000, 90000], 1), (1, [PRIOR, 89000, 90000], 1),
    (3, [PRIOR, 90000, 89000], 2), (3, [PRIOR, 90000, 90000], 1),
    # the margin is the PRIOR's: a challenger inside it does not become the bar for the next one
    (1, [PRIOR, 99000, 98500], 0), (1, [PRIOR, 99000, 97900], 2), (1, [PRIOR, 97900, 97000, 97500], 2),
    (3, [PRIOR, 97000, 95100], 0), (3, [PRIOR, 97000, 94900], 2),
    (1, [PRIOR, 101000, 150000, 99999, 120000, 98001], 0), (1, [PRIOR, 101000, 150000, 99999, 120000, 97999], 5),
])
def test_margin(sim, in_flight, costs, keeps):
    cand = CANDS[:len(costs)]
    ran, (got, cost, chosen) = decide(sim, cand, costs, in_flight)
    assert got == cand and [float(c) for c in cost] == [float(ms(c)) for c in costs]
    assert chosen == keeps
    trial = len(schedule(cand, in_flight, 0 if in_flight == 1 else in_flight))
    assert ran[trial:] == [cand[keeps]] * (len(ran) - trial)


# ---- trials that can never be evaluated ------------------------------------------------------------------------------------------
def test_a_span_that_never_arrives_ends_the_trial_65_launches_later(sim):
    cand = CANDS[:2]
    costs = {17: 9000, 6: 5000}
    silent = settle_of(1) + 3 + 1  # the second candidate's second launch

    def records(f, step):
        return (None, 0) if step == silent else one_at_a_time(costs)(f, step)
    for f in schedule(cand, 1):
        assert sim.frame(8, cand, records) == f
    last = sim.head() - 1
    assert sim.launches(8)[0][1, 2] == last
    while sim.head() <= last + 64:
        assert sim.frame(8, cand, records) == 17
        assert sim.choice(8)[2] == -1
    assert sim.head() == last + 65
    assert sim.frame(8, cand, records) == 17
    _, cost, chosen = sim.choice(8)
    assert chosen == 0 and not cost.any()
    assert [sim.frame(8, cand, records) for _ in range(5)] == [17] * 5


@pytest.mark.parametrize("apart, evaluated", [(255, True), (256, False), (300, False)])
def test_a_trial_spread_over_the_whole_ring_keeps_the_prior(sim, apart, evaluated):
    """Launches of other shapes between a trial's: once the coming launch is kRing or more past the trial's first, the first slots
    are (about to be) somebody else's -- the prior stays and no cost is reported; one launch fewer and the trial is read as usual."""
    assert sim.lib.td_ring() == 256
    cand = CANDS[:2]
    rec = one_at_a_time({17: 9000, 6: 5000})
    want = schedule(cand, 1)
    for k, f in enumerate(want):
        if k == len(want) - 1:  # before the trial's last launch: other shapes' launches, measured and faster than anything
            first = sim.launches(8)[0][0, 0]
            while sim.head() + 1 - first < apart:
                sim.launch(17, 1)
        assert sim.frame(8, cand, rec) == f
    assert sim.head() - first == apart
    assert sim.frame(8, cand, rec) == (6 if evaluated else 17)
    _, cost, chosen = sim.choice(8)
    if evaluated:
        assert chosen == 1 and [float(c) for c in cost] == [float(ms(9000)), float(ms(5000))]
    else:
        assert chosen == 0 and not cost.any()


# ---- re-opening --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ref, now, reopens", [
    (103, 78, False), (103, 77, True), (103, 128, False), (103, 129, True), (103, 103, False),
    (100, 75, False), (100, 74, True), (100, 125, False), (100, 126, True),
    (3, 3, False), (3, 2, True), (3, 4, True),        # (a quarter of 3 is 0: any change re-opens)
    (103, 0, False), (0, 5000, False), (0, 0, False),  # never while either chain is unknown
    (4000, 1 << 24, True), (1 << 24, 3 << 22, False), (1 << 24, (3 << 22) - 1, True),
])
def test_reopening_on_the_integer_quarter_bounds(sim, ref, now, reopens):
    cand = CANDS[:3]
    costs = [PRIOR, 80000, 90000]
    ran, (_, cost, chosen) = decide(sim, cand, costs, chain=ref)
    assert chosen == 1 and ran[-1] == 6 and sim.launches(11)[2] == ref
    rec = one_at_a_time(dict(zip(cand, [70000, 90000, 60000])))
    # the call that re-opens already runs the kept kernel as the first of the new trial's settling launches
    sim.mark()
    ran = [sim.frame(11, cand, rec, chain=now) for _ in range(4 + 9 + 1)]
    got, cost2, chosen2 = sim.choice(11)
    if not reopens:
        assert ran == [6] * len(ran) and got == cand and chosen2 == 1 and np.array_equal(cost, cost2)
        return
    assert got == [6, 17, 18]  # the kept kernel first, the others in the caller's order
    assert ran == schedule(got, 1) + [18]
    assert chosen2 == 2 and [float(c) for c in cost2] == [float(ms(c)) for c in (90000, 70000, 60000)]
    assert sim.launches(11)[2] == now


# ---- keys, candidate sets, shapes, slots ------------------------------------------------------------------------------------------
def test_same_key_with_another_candidate_set_starts_over_from_its_first(sim):
    cand = [17, 6, 12]
    ran, (_, _, chosen) = decide(sim, cand, [PRIOR, 80000, 90000])
    assert chosen == 1
    rec = one_at_a_time({17: PRIOR, 6: 80000, 12: 90000, 18: 70000})
    # the same set in another order is the same set: nothing happens
    assert [sim.frame(11, [6, 12, 17], rec) for _ in range(3)] == [6, 6, 6] and sim.choice(11)[0] == cand
    # one member fewer: a fresh trial from ITS cand[0], not from what was kept
    ran = [sim.frame(11, [17, 12], rec) for _ in range(4 + 6 + 1)]
    assert ran == schedule([17, 12], 1) + [12] and sim.choice(11)[0] == [17, 12] and sim.choice(11)[2] == 1
    # as many members, one of them another
    ran = [sim.frame(11, [17, 18], rec) for _ in range(4 + 6 + 1)]
    assert ran == schedule([17, 18], 1) + [18] and sim.choice(11)[0] == [17, 18]
    assert sum(1 for k in sim.slots() if k) == 1
    # a trial that a moved chain re-opened lists the kept kernel first: a changed set still starts from the CALLER's first
    assert sim.launches(11)[2] == 0 and sim.choice(11)[2] == 1  # (18 kept; the chain was unknown when it was chosen)
    sim.mark()
    ran, (got, _, chosen) = decide(sim, [17, 6, 18], [PRIOR, 90000, 70000], chain=100)
    assert got == [17, 6, 18] and chosen == 2
    assert sim.frame(11, [17, 6, 18], rec, chain=200) == 18 and sim.choice(11)[0] == [18, 17, 6]
    sim.mark()
    ran = [sim.frame(11, [17, 6], rec, chain=200) for _ in range(4 + 6 + 1)]
    assert ran == schedule([17, 6], 1) + [6] and sim.choice(11)[0] == [17, 6]


def test_a_new_key_of_a_known_shape_starts_from_what_that_shape_kept(sim):
    cand = [17, 6, 12]
    S, T = 0x51, 0x71
    decide(sim, cand, [PRIOR, 80000, 90000], key=21, shape=S)   # keeps 6
    decide(sim, cand, [PRIOR, 90000, 80000], key=23, shape=S)   # (starts from 6) keeps 12
    decide(sim, cand, [PRIOR, 90000, 95000], key=25, shape=T)   # another shape: keeps 6
    assert [sim.choice(k)[2] for k in (21, 23, 25)] == [1, 2, 1] and sim.choice(23)[0] == [6, 17, 12]
    rec = one_at_a_time({17: PRIOR, 6: 80000, 12: 90000, 18: 70000})
    # an undecided trial of the shape says nothing, however recently it was used (six candidates, 6 among them)
    rec6 = one_at_a_time(dict(zip(CANDS, [PRIOR] * 6)))
    for _ in range(6):
        sim.frame(27, CANDS, rec6, shape=S)
    assert sim.choice(27)[0] == [12, 17, 6, 18, 16, 10] and sim.choice(27)[2] == -1  # (itself started from 23's 12)
    # the most recently USED decided trial of the shape: 23 (kept 12) ...
    assert sim.frame(31, cand, rec, shape=S) == 12 and sim.choice(31)[0] == [12, 17, 6]
    # ... and after 21 has been used again, 21 (kept 6)
    assert sim.frame(21, cand, rec, shape=S) == 6
    assert sim.frame(33, cand, rec, shape=S) == 6 and sim.choice(33)[0] == [6, 17, 12]
    # what it kept is no candidate any more: the next most recent whose kernel is, else cand[0]
    assert sim.frame(35, [17, 12, 18], rec, shape=S) == 12 and sim.choice(35)[0] == [12, 17, 18]
    assert sim.frame(37, [17, 18], rec, shape=S) == 17 and sim.choice(37)[0] == [17, 18]
    # an unknown shape: cand[0]
    assert sim.frame(39, cand, rec, shape=0x91) == 17


def test_a_ninth_key_recycles_the_least_recently_used_slot_and_no_other(sim):
    cand = [17, 6]
    rec = one_at_a_time({17: 900, 6: 800})
    keys = [101 + 2 * i for i in range(8)]
    for k in keys:
        sim.frame(k, cand, rec, shape=k)
    assert sim.slots() == keys
    for k in (keys[3], keys[0], keys[7], keys[1], keys[2], keys[4], keys[6]):  # keys[5] is now the least recently used
        sim.frame(k, cand, rec, shape=k)
    before = {k: (sim.choice(k), sim.launches(k)[0].copy()) for k in keys}
    sim.frame(999, cand, rec, shape=999)
    want = list(keys)
    want[5] = 999
    assert sim.slots() == want and sim.choice(keys[5]) is None
    for k in keys:
        if k != keys[5]:
            assert sim.choice(k)[0] == before[k][0][0] and np.array_equal(sim.launches(k)[0], before[k][1])
    sim.frame(1001, cand, rec, shape=1001)  # the next victim: keys[3], used longest ago of the rest
    want[3] = 1001
    assert sim.slots() == want


@pytest.mark.parametrize("in_flight", [1, 3])
def test_interleaved_shapes_read_only_their_own_launches(sim, in_flight):
    """Two keys take turns (and a third, single-candidate shape launches in between): each trial's costs are its own launches'."""
    cand = CANDS[:3]
    lag = 0 if in_flight == 1 else in_flight
    costs = {5: [60000, 40000, 50000], 7: [30000, 45000, 29000]}
    if in_flight == 1:
        recs = {}
        for key in costs:
            by_f = dict(zip(cand, costs[key]))
            # (one_at_a_time counts this key's own frames: every third launch of the script)
            recs[key] = (lambda base: lambda f, step: base(f, step // 3))(one_at_a_time(by_f))
        shared = None
    else:
        shared = Clock({}, wobble=lambda step: (step * 7919) % 1013)  # one device clock: a launch ends its own cost after the launch before it, whoever that was
    n = settle_of(in_flight) + 3 * per_of(in_flight) + lag + 2
    for _ in range(n):
        for key in (5, 7):
            if shared:
                shared.costs = dict(zip(cand, costs[key]))
                sim.frame(key, cand, shared, lag=3 * lag, in_flight=in_flight, shape=key)
            else:
                sim.frame(key, cand, recs[key], lag=lag, in_flight=in_flight, shape=key)
        sim.launch(3, sim.log[-1][3] + 2 if shared else 1, 3 * lag)
        if shared:
            shared.now += 2
    for key in (5, 7):
        got, cost, chosen = sim.choice(key)
        want = []
        mine = [r for r in sim.log if r[4] == key][settle_of(in_flight):]
        per, f = per_of(in_flight), in_flight
        for i in range(3):
            turn = mine[i * per:(i + 1) * per]
            assert [r[0] for r in turn] == [cand[i]] * per
            assert np.array_equal(sim.launches(key)[0][i, :per], [r[1] for r in turn])
            w = ms(min(r[2] for r in turn[1:])) if in_flight == 1 else ms((turn[per - f][3] - turn[f][3]) / np.float64(per - 2 * f))
            assert cost[i].tobytes() == w.tobytes(), (key, i)
            want.append(w)
        assert chosen == kept(want, in_flight) and len({float(w) for w in want}) == 3, (key, cost)
    assert sim.choice(5)[2] != 0 and list(sim.choice(5)[1]) != list(sim.choice(7)[1])


# ---- a kernel-times reset in the middle of a trial -------------------------------------------------------------------------------
def reset_script(lib, in_flight, reset_after, rewind=False):
    """One script, whatever the reset does: the records are a function of the flavour and of the frame's place in the script."""
    cand = CANDS[:3]
    by_f = dict(zip(cand, [PRIOR, 90000, 80000]))
    records = one_at_a_time(by_f) if in_flight == 1 else Clock(by_f, wobble=lambda step: (step * 31) % 17)
    lag = 0 if in_flight == 1 else in_flight
    s = Sim(lib, rewind)
    try:
        ran = []
        for k in range(settle_of(in_flight) + 3 * per_of(in_flight) + lag + 4):
            ran.append(s.frame(13, cand, records, lag=lag, in_flight=in_flight))
            if k == reset_after:
                s.reset()
                assert s.lib.td_reported(s.h) == 0
        got, cost, chosen = s.choice(13)
        return ran, got, cost.tobytes(), chosen
    finally:
        s.close()


@pytest.mark.parametrize("in_flight", [1, 3])
def test_reset_mid_trial_changes_neither_choice_nor_costs(lib, in_flight):
    """vr_reset_kernel_times behind any launch of a trial -- settling, any turn, waiting, after the choice -- leaves what runs, the
    choice and the costs exactly what the script gives without a reset.  (bench.py resets between warm-up and the timed frames.)"""
    plain = reset_script(lib, in_flight, None)
    assert plain[3] == 2 and plain[0][-1] == 18
    for k in range(len(plain[0])):
        assert reset_script(lib, in_flight, k) == plain, k


@pytest.mark.parametrize("in_flight", [1, 3])
def test_the_reset_case_sees_a_counter_that_rewinds(lib, in_flight):
    """The same comparison against a context whose reset sets the launch counter back to 0 (what vr_reset_kernel_times did while the
    trials stored LastLaunch::ring_head and the reset rewound it): launches after the reset take the numbers, and the ring slots, of
    the trial's earlier launches, and the trial reads their records as its own.  The comparison above must not pass there."""
    plain = reset_script(lib, in_flight, None, rewind=True)
    assert plain == reset_script(lib, in_flight, None)
    wrong = [k for k in range(len(plain[0])) if reset_script(lib, in_flight, k, rewind=True) != plain]
    assert wrong, "a rewinding reset went unnoticed at every point of the trial"
    # a reset right behind the first candidate's last trial launch: the other candidates' launches land in its slots
    assert settle_of(in_flight) + per_of(in_flight) - 1 in wrong
