"""GPU, two ranks on one card (gloo): a GradGuard per phase under data parallelism.  guard.measure() reduces the bucket first and measures the averaged
gradient, so one rank's inf reaches every rank's measurement and all of them skip the same step.  The ranks are fresh child processes."""
import json
import math
import os
import socket
import struct
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def test_one_ranks_inf_skips_the_step_on_every_rank(tmp_path):
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    outs = [str(tmp_path / f"guard{r}.json") for r in range(2)]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "grad_guard_dp_worker.py"), str(r), "2", str(port), outs[r]], env=env) for r in range(2)]
    try:
        for p in procs:
            assert p.wait(timeout=600) == 0
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    a, b = [json.load(open(o)) for o in outs]
    for r in (a, b):
        assert r["skipped_total"] == [0.0, 1.0], r                      # D guard never, G guard once
        assert r["skipped"] == [[0.0, 0.0], [0.0, 1.0], [0.0, 0.0]], r
        assert all(abs(s - 0.5) < 1e-12 for s in r["grad_scale"]), r
        assert r["replicas_identical"], r
        assert r["gen_moved"][0] > 0.9 and r["gen_moved"][1] == 0.0 and r["gen_moved"][2] > 0.9, r      # the skipped G phase moved nothing; the third iteration updates normally
        assert all(m > 0.9 for m in r["dis_moved"]), r
        assert r["gen_steps"] == [[4], [2]], r                          # ggen is stepped twice per measurement; the skipped one advanced no count
    # every rank measured the same reduced bits: identical norms, and finite wherever nothing was skipped
    assert a["norm_bits"] == b["norm_bits"], (a["norm_bits"], b["norm_bits"])
    for it, row in enumerate(a["norm_bits"]):
        for ph, w in enumerate(row):
            v = struct.unpack("f", struct.pack("i", w))[0]
            assert (it, ph) == (1, 1) or (math.isfinite(v) and v > 0.0), (it, ph, v)
