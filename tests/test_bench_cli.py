"""bench.py's one-GPU command line: a plain run measures the headline only, `--full` adds every other leg, and
`--dump-outputs DIR` saves what the last timed step returned, identical from run to run with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests._util import load_json

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def _bench(*args, timeout=600):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + list(args),
                         capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


def test_dump_outputs_keeps_float32_widens_the_rest_and_caps_the_size(tmp_path):
    import bench
    bench.dump_outputs(str(tmp_path / "d"), {"a": np.arange(3, dtype=np.float32), "b": np.arange(4), "c": np.float64(2.5)})
    a, b, c = (np.load(str(tmp_path / "d" / (k + ".npy"))) for k in "abc")
    assert a.dtype == np.float32 and b.dtype == np.float64 and c.dtype == np.float64
    assert a.tolist() == [0.0, 1.0, 2.0] and b.tolist() == [0.0, 1.0, 2.0, 3.0] and float(c) == 2.5
    with pytest.raises(ValueError):
        bench.dump_outputs(str(tmp_path / "big"), {"x": np.zeros((64 << 20) // 8 + 1)})
    assert not os.path.exists(str(tmp_path / "big"))


@pytest.mark.gpu
def test_plain_run_is_the_headline_and_dumps_the_last_step(device, tmp_path):
    runs = []
    for r in range(2):
        d = _bench("--workload", "c1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / str(r)))
        runs.append((d, np.load(str(tmp_path / str(r) / "lml.npy"))))
    d, lml = runs[0]
    assert all(d[k] is not None for k in HEADLINE) and d["steps"] == 3 and d["warmup"] == 1
    assert d["unit"] == "LML evals/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert abs(d["value"] * d["ms_per_step"] - 1e3) < 1e-6 * 1e3
    assert not any(k.startswith("roofline") or k in ("cpu_baseline", "loss_backward", "notes") for k in d)
    assert lml.dtype == np.float64 and float(lml) == d["lml"]
    case = [c for c in load_json("lml_cases.json") if c["name"] == "C1_rbf_512_2"][0]
    assert abs(float(lml) - case["lml"]) < 1e-8
    assert np.array_equal(runs[1][1], lml)                 # same arguments, same inputs: the same output


@pytest.mark.gpu
def test_full_run_keeps_the_other_legs(device):
    d = _bench("--workload", "c1", "--steps", "2", "--warmup", "1", "--full", "--no-cpu-baseline")
    assert all(d[k] is not None for k in HEADLINE) and d["steps"] == 2
    assert "roofline" in d and "loss_backward" in d
    assert d["loss_backward"]["ms_per_step"] > 0
