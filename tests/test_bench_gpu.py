"""GPU: a plain `bench.py` run times the headline only — --steps timed steps, none of the --full keys filled — and --dump-outputs writes
the last timed step's losses (those of the result line) and model state."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_dumps_its_last_step(tmp_path):
    d = tmp_path / "out"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--batch", "4", "--steps", "3", "--warmup", "1", "--dump-outputs", str(d)],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    r = json.loads(lines[0])
    assert r["steps"] == 3 and r["warmup"] == 1 and r["ms_per_step"] > 0 and r["value"] > 0 and r["dtype"] == "f32"
    assert r["cpu_baseline"] is None and r["minimal_schedule"] is None and r["as_trainer"] is None and r["secondary_precisions"] is None
    assert r["roofline"]["dominant_kernel"] is None
    for k, v in r["losses_last_step"].items():
        got = np.load(d / f"{k}.npy")
        assert got.dtype == np.float64 and got[0] == v, k
    files = os.listdir(d)
    assert sorted(f for f in files if f.startswith("state_")) == [f"state_{n}.npy" for n in ("cgen", "gdis", "ggen", "idis", "vdis")]
    assert sum(os.path.getsize(d / f) for f in files) <= 64 * 10**6
    for f in files:
        a = np.load(d / f)
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), f
