"""GPU: a plain `bench.py` run prints the headline line and nothing of `--full`, and `--dump-outputs DIR` writes what
its last timed step computed (every loss term, the total, sampled parameters and gradients) as float32 .npy files --
the same bits in two runs with the same arguments."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def _run(out):
    env = {k: v for k, v in os.environ.items() if k != "EFG_DETERMINISTIC"}
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "2", "--warmup", "1", "--points", "30000",
                        "--queries", "100", "--scenes", "1", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0]), {os.path.basename(p)[:-4]: np.load(p) for p in glob.glob(str(out / "*.npy"))}


def test_plain_run_and_dump_outputs(dev, tmp_path):
    line, files = _run(tmp_path / "a")
    assert line["steps"] == 2 and line["higher_is_better"] is True and line["unit"] == "scenes/s"
    assert line["dtype"] == "f32" and line["value"] == pytest.approx(1000.0 / line["ms_per_step"], rel=1e-6)
    assert line["deterministic"] is True
    # the 2 steps were timed: the one rank's own time per step is the headline's, and issuing them took no longer
    assert line["rank_ms_per_step"]["all"] == [pytest.approx(line["ms_per_step"], abs=1e-3)]
    assert 0 < line["host_issue_ms_per_step"] <= line["ms_per_step"] * 1.001
    for key in ("roofline", "kernels", "cpu_baseline", "steady_state", "full_graph", "arm_bf16x3", "yaml_config",
                "host_own_ms_per_step", "streamk_fallbacks"):
        assert key not in line, key
    assert {"total_loss", "params", "grads"} <= set(files) and sum(k.startswith("loss") for k in files) >= 30
    assert sum(a.nbytes for a in files.values()) <= 64 << 20
    for name, a in files.items():
        assert a.dtype == np.float32 and np.isfinite(a).all(), name
    assert files["total_loss"].size == 1 and files["params"].size == files["grads"].size > 0
    assert np.abs(files["grads"]).max() > 0
    # the same arguments, a second process: the same inputs and the same bits out
    _, again = _run(tmp_path / "b")
    assert set(again) == set(files)
    differ = [k for k in sorted(files) if not np.array_equal(files[k], again[k])]
    assert not differ, differ
