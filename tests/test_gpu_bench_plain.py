"""bench.py without --full: the headline alone.  It prints the contract's line from the W + K resident steps, decrypt-checks
them and writes --dump-outputs, and runs none of the legs that --full adds (CPU baseline, host-buffer legs, secondary
workloads, live PMC passes): a plain run spends little time outside its steps."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_is_the_headline_alone(built_lib, tmp_path):
    steps, warmup = 5, 2
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup",
                        str(warmup), "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=300, cwd=ROOT)
    wall = time.perf_counter() - t0
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and len(r.stdout.splitlines()) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["metric"] == "gate bootstraps/sec (HomNAND)" and d["unit"] == "gate bootstraps/s" and d["dtype"] == "f64"
    assert d["higher_is_better"] is True and d["n_gpus"] == 1 and d["steps"] == steps and d["warmup"] == warmup
    assert d["full"] is False and d["decrypt_ok"] is True
    assert d["value"] == pytest.approx(1024 / (d["ms_per_step"] * 1e-3), rel=2e-3)
    assert d["roofline"]["avg_launch_ms"] > 0 and "traffic_live" not in d["roofline"]     # no PMC passes
    for k in ("cpu_baseline", "secondary", "wallclock_gates_per_s", "pipelined_gates_per_s", "paths_bit_identical"):
        assert k not in d, k
    # the dump is the timed batch: 1024 NANDs of the seeded inputs (rank 0's stream, seed 1000)
    rng = np.random.default_rng(1000)
    b0, b1 = rng.integers(0, 2, 1024), rng.integers(0, 2, 1024)
    assert d["dumped_outputs"]["rows"] == 1024
    assert np.array_equal(np.load(tmp_path / "bits.npy"), 1 - (b0 & b1))
    # what the run spends outside its W + K steps: set-up, pre-flight, the decrypt check, the dump, start and exit
    assert wall - (steps + warmup) * d["ms_per_step"] * 1e-3 < 30.0, wall
