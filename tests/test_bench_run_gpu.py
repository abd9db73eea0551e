"""bench.py end to end on a small configuration (C1), in fresh child processes: a plain run prints the headline line and nothing
it does not need, --full adds the other legs; both time the same serial leg of the same scene."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONTRACT = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("overlapped", "roofline", "sync_8d", "arith_ab", "serial_with_present")


def run_bench(*argv):
    cmd = [sys.executable, *(["-s"] if sys.flags.no_user_site else []), os.path.join(ROOT, "bench.py"),
           "--workload", "C1", "--steps", "3", "--warmup", "2", *argv]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_is_the_headline_alone(tmp_path):
    out = run_bench("--dump-outputs", str(tmp_path))
    assert all(k in out for k in CONTRACT)
    assert out["metric"] == "Gsamples/s" and out["unit"] == "Gsamples/s" and out["higher_is_better"] is True and out["dtype"] == "f32"
    assert out["value"] == out["serial"]["value"] > 0 and out["ms_per_step"] == out["serial"]["ms_per_step"] > 0
    assert out["steps"] == 3 and out["warmup"] == 2
    assert not any(k in out for k in FULL_ONLY + ("parity", "cpu_baseline", "full_turn", "regimes"))
    frame, counters = np.load(tmp_path / "frame.npy"), np.load(tmp_path / "counters.npy")
    assert frame.dtype == np.float32 and frame.shape[-1] == 4 and counters.dtype == np.float64 and counters.shape == (3,)
    assert counters[0] > 0


def test_full_run_adds_the_other_legs():
    plain = run_bench()
    full = run_bench("--full", "--no-cpu-baseline", "--no-live-pmc", "--no-regimes", "--turn-frames", "0")
    assert all(k in full for k in CONTRACT + FULL_ONLY)
    assert full["overlapped"]["frames_of_batched_launches_equal_single_renders"] is True
    # the same scene and the same timed cameras: what the serial leg composited does not depend on --full
    assert full["serial"]["composited_samples_timed"] == plain["serial"]["composited_samples_timed"]
    for k in ("workload", "composited_samples_frame0", "fetched_samples_frame0", "covered_pixels_frame0"):
        assert full["config"][k] == plain["config"][k], k
