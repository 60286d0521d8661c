"""bench.py's command line: a plain run measures the headline only and can write the last timed step's
outputs (--dump-outputs); --full brings back the roofline figures behind it."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus"}
FULL_ONLY = {"roofline", "roofline_kernels", "stage_roofline", "step_roofline", "perturber_roofline", "parity_mode",
             "cpu_baseline"}


def _bench(*args):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2", *args]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


def test_plain_run_is_headline_only_and_dumps_outputs(tmp_path):
    d = str(tmp_path / "out")
    res = _bench("--dump-outputs", d)
    assert HEADLINE <= set(res) and not (FULL_ONLY & set(res)), sorted(res)
    assert res["steps"] == 3 and res["warmup"] == 2 and res["unit"] == "frames/s" and res["dtype"] == "bf16"
    # value = frames per second of the timed steps, ms_per_step = their wall time / steps (batch 6, one GPU)
    assert res["value"] == pytest.approx(6 * 1000.0 / res["ms_per_step"], rel=2e-3)
    files = sorted(glob.glob(os.path.join(d, "*.npy")))
    names = {os.path.basename(f)[:-4] for f in files}
    assert "log.loss" in names and any(n.startswith("param.") for n in names), sorted(names)[:8]
    assert sum(os.path.getsize(f) for f in files) <= 64 << 20
    for f in files:
        x = np.load(f)
        assert x.dtype == np.float32 and x.size > 0 and np.isfinite(x).all(), f


def test_full_run_adds_the_roofline_figures():
    res = _bench("--full", "--no-cpu-baseline", "--no-parity-mode")
    assert HEADLINE <= set(res), sorted(res)
    assert {"roofline", "roofline_kernels", "stage_roofline", "step_roofline", "perturber_roofline"} <= set(res)
    assert "cpu_baseline" not in res and "parity_mode" not in res
