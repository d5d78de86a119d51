"""A plain ``bench.py`` run (no --full): --steps timed steps of the headline mode, a line that carries the headline figure and
none of --full's legs, and --dump-outputs writing what the last timed step returned."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu


def test_plain_run_times_its_steps_and_dumps_the_last_one(tmp_path, gpu_device):
    out = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--points", "20000",
           "--dump-outputs", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=REPO)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["dtype"] == "f16x8c" and d["unit"] == "normals/sec" and d["higher_is_better"]
    assert d["value"] > 0 and abs(d["value"] * d["ms_per_step"] / 1e3 / 20000 - 1) < 1e-9        # one step = one 20k cloud
    assert d["gate_cascade"]["queries"] == 3 * 20000 and d["x8_guard"]["queries"] == 3 * 20000     # the counters of the timed steps
    moved = {"roofline", "single_stream", "parity", "exact_mode", "fast_mode", "full_pair_mode", "pair_cascade_mode", "x8_e4m3_mode",
             "mups", "strong", "strong_projection", "rms_angle_error_deg", "cpu_baseline"}
    assert not moved & set(d), moved & set(d)
    normals, expert, probs = (np.load(out / (k + ".npy")) for k in ("normals", "expert", "probs"))
    assert normals.dtype == expert.dtype == probs.dtype == np.float32
    assert normals.shape == (20000, 3) and expert.shape == (20000,) and probs.shape == (20000, 7)
    assert np.all(np.isfinite(normals)) and np.allclose(probs.sum(1), 1, atol=1e-4)
    assert np.array_equal(np.bincount(expert.astype(np.int64), minlength=7), d["config"]["routing_histogram"])
