"""GPU, two ranks on one card (gloo): a GradGuard per phase under data parallelism.  guard.measure() reduces the bucket first and measures the averaged
gradient, so one rank's inf reaches every rank's measurement and all of them skip the same step.  The ranks are fresh child processes."""
import math
import struct

import pytest

from tests import rig

pytestmark = pytest.mark.gpu


def test_one_ranks_inf_skips_the_step_on_every_rank(tmp_path):
    a, b = rig.run_ranks("grad_guard_dp_worker.py", tmp_path, tag="guard", timeout=600)
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
