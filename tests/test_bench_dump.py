"""bench.py --dump-outputs: the writer (size limit, seeded sample, dtypes) and the argument checks (CPU only: nothing here
touches a GPU)."""
import importlib.util
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def load_bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(os.path.dirname(HERE), "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_small_outputs_are_written_whole(tmp_path):
    bench = load_bench()
    frame = np.arange(6 * 5 * 4, dtype=np.float32).reshape(6, 5, 4)
    counters = np.array([7.0, 3.0, 9.0])
    shapes = bench.dump_outputs(str(tmp_path / "out"), {"frame": frame, "counters": counters})
    assert shapes == {"frame": [6, 5, 4], "counters": [3]}
    got = np.load(tmp_path / "out" / "frame.npy")
    assert got.dtype == np.float32 and np.array_equal(got, frame)
    got = np.load(tmp_path / "out" / "counters.npy")
    assert got.dtype == np.float64 and np.array_equal(got, counters)


def test_large_output_is_a_fixed_seeded_sample_within_the_limit(tmp_path):
    bench = load_bench()
    frame = np.random.default_rng(5).random((300, 200, 4), dtype=np.float32)  # 960000 bytes
    counters = np.array([1.0, 2.0, 3.0])
    limit = 100_000
    bench.dump_outputs(str(tmp_path / "a"), {"frame": frame, "counters": counters}, limit=limit)
    bench.dump_outputs(str(tmp_path / "b"), {"frame": frame.copy(), "counters": counters}, limit=limit)
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= limit
    a, b = np.load(tmp_path / "a" / "frame.npy"), np.load(tmp_path / "b" / "frame.npy")
    assert a.dtype == np.float32 and a.shape[1] == 4 and 0 < a.shape[0] < 300 * 200
    assert np.array_equal(a, b)                                   # same sample every run
    rows = frame.reshape(-1, 4)
    idx = np.sort(np.random.default_rng(0).choice(len(rows), size=a.shape[0], replace=False))
    assert np.array_equal(a, rows[idx])                          # whole pixels, in index order
    assert np.array_equal(np.load(tmp_path / "a" / "counters.npy"), counters)


def test_only_float_outputs(tmp_path):
    bench = load_bench()
    with pytest.raises(TypeError):
        bench.dump_outputs(str(tmp_path), {"counters": np.array([1, 2, 3], dtype=np.uint64)})


@pytest.mark.parametrize("argv", [["--steps", "0"], ["--gpus", "2", "--dump-outputs", "x"]])
def test_arguments_refused_before_any_gpu_call(monkeypatch, argv):
    bench = load_bench()
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 2
