"""bench.py as the driver runs it: a plain `--gpus 1 --steps K --warmup W` run times the headline and nothing else, and
`--dump-outputs DIR` writes what the timed call returned — the same arrays from run to run, whatever number of iterations
the clock-limited spin-up ran."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(*extra):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + list(extra),
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-3000:]
    return lines[0]


@pytest.mark.parametrize("extra", [[], ["--workload", "cfg5", "--samples", "8"]])
def test_plain_run_times_the_headline_only_and_dumps_the_same_outputs_twice(tmp_path, extra):
    steps = 30
    lines = [run_bench("--steps", str(steps), "--warmup", "3", "--dump-outputs", str(tmp_path / tag), *extra) for tag in "ab"]
    for line in lines:
        assert line["steps"] == steps and line["ms_per_step"] > 0 and line["value"] > 0 and line["all_finite"]
        assert line["unit"] == "it/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
        assert not any(k in line for k in ("other_configs", "cpu_baseline", "cold_start", "value_alt"))
        assert line["roofline"]["traffic"] is None
    for name in ("loss_curve", "finite", "params"):
        a, b = (np.load(str(tmp_path / tag / (name + ".npy"))) for tag in "ab")
        assert a.dtype == np.float32 and a.shape == b.shape
        assert np.array_equal(a, b), (name, float(np.abs(a - b).max()))
    curve = np.load(str(tmp_path / "a" / "loss_curve.npy"))
    assert curve.shape == (steps,) and np.isfinite(curve).all()
    assert (np.load(str(tmp_path / "a" / "finite.npy")) != 0).all()
