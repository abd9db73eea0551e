"""tools/resample_bench.py: its geometry helper on the CPU, and one rehearsal run of the tool itself on a small volume on the GPU."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_rotation_keeps_the_centre_and_turns_x_towards_y():
    import resample_bench as rb
    m = rb.rotation_z(10.0, (255.5, 255.5, 255.5))
    assert m.shape == (3, 4)
    c = np.array([255.5, 255.5, 255.5])
    assert np.allclose(m[:, :3] @ c + m[:, 3], c) and np.allclose(m[:, :3] @ m[:, :3].T, np.eye(3))
    p = m[:, :3] @ (c + [1.0, 0.0, 0.0]) + m[:, 3] - c
    assert np.allclose(p, [np.cos(np.radians(10.0)), np.sin(np.radians(10.0)), 0.0])


@pytest.mark.gpu
def test_resample_bench_rehearsal(tmp_path):
    """The tool on a 64^3 rehearsal of C4: every leg and form reports, the forms agree, out[1] + out[2] == out[0], and the file holds
    the lines that were printed."""
    out = tmp_path / "bench.json"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "resample_bench.py"), "--workload", "C4", "--vol-n", "64", "--steps", "1",
                        "--warmup", "0", "--no-cpu", "--out", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert [json.loads(l) for l in out.read_text().splitlines()] == lines
    legs = [l for l in lines if "leg" in l]
    assert len(legs) == 8 and {l["leg"][0] for l in legs} == {"a", "b", "c"} and {l["form"] for l in legs} == {"default", "plain"}
    for l in legs:
        assert l["equals_first_form"] and l["loaded"] + l["unloaded"] == l["box"] == l["inside"] + l["outside"] and l["inside"] > 0
        assert l["kernel_ms"] > 0.0 and l["refresh_ms"] > 0.0 and l["must_write_bytes"] == l["box"] * 4 * bin(l["channels"]).count("1")
        if l["form"] == "plain":
            assert l["loaded"] == l["inside"]
    assert sum("case" in l for l in lines) == 3
