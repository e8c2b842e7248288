"""GPU, two ranks on one card (gloo): the LeCam anchors under data parallelism.  Between its two launches the batch sums are all-reduced (SUM, n_dis x 4 doubles)
over the feature's own process group, so every rank holds the anchors of one process that sees the concatenated logits, and the replicas stay bit-identical, as
they are without the feature.  The logits of the first leg are multiples of 2^-8 below 8 in magnitude, so every sum is exact in any order
(tests/test_lecam_cpu.py::test_exact_logits_sum_exactly).  The two ranks are fresh child processes, started once for this module; the parent waits for each with a
limit, kills leftovers, never retries."""
import numpy as np
import pytest

from tests import rig
from tests import test_lecam_cpu as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ranks(tmp_path_factory):
    return rig.run_ranks("lecam_dp_worker.py", tmp_path_factory.mktemp("lecam_dp"), tag="lecam", timeout=300)


def test_every_rank_holds_the_anchors_of_one_process_on_the_concatenated_logits(ranks):
    from tests.lecam_dp_worker import ITERATIONS, RULE, logits
    a, b = ranks
    want, state = [], R.zero_state(3)
    for it in range(ITERATIONS):
        (r0, f0), (r1, f1) = logits(it, 0), logits(it, 1)
        yr, yf = [np.concatenate(p) for p in zip(r0, r1)], [np.concatenate(p) for p in zip(f0, f1)]
        sums = R.sums_ref(yr, yf)
        assert np.array_equal(sums, R.sums_ref(r0, f0) + R.sums_ref(r1, f1))      # exact logits: the ranks' sums add up to the concatenation's, bit for bit
        z = lambda ys: [np.zeros_like(y) for y in ys]
        state, _, _, _, _ = R.apply_ref(yr, yf, sums, state, RULE["decay"], RULE["start"], RULE["weight"], RULE["one_sided"], [np.float32(0)] * 3, z(yr), z(yf))
        want.append(state)
    print(f"\n[lecam dp] anchors after three iterations {[(float(R.bits_f32(s[0])), float(R.bits_f32(s[1]))) for s in a['states'][-1]]}; regs {a['regs']} / {b['regs']}")
    assert a["states"] == b["states"] == want
    assert [s[R.UPDATES] for s in a["states"][-1]] == [3, 3, 3] and [s[R.ACTIVE] for s in a["states"][-1]] == [1, 1, 1]
    assert a["anchor_collectives"] == b["anchor_collectives"] == ITERATIONS      # one collective per iteration
    assert a["regs"] != b["regs"]                                                 # the 1 / n of the regulariser stays the rank's own


def test_replicas_stay_bit_identical_in_the_iteration(ranks):
    a, b = ranks
    print(f"\n[lecam dp step] weights {[h[:8] for h in a['weights_sha']]}, state {a['step_state']}, regs {a['step_regs']} / {b['step_regs']}")
    assert a["data_sha"] != b["data_sha"]      # distinct data
    assert a["weights_sha"] == b["weights_sha"] and len(set(a["weights_sha"])) == 3
    assert a["step_state"] == b["step_state"] and [s[R.UPDATES] for s in a["step_state"]] == [2, 2, 2] and [s[R.ACTIVE] for s in a["step_state"]] == [1, 1, 1]
    assert a["step_collectives"] == b["step_collectives"] == 2 and a["finite"] and b["finite"]
    assert all(v == 0.0 for v in a["step_regs"][0] + b["step_regs"][0])      # the first iteration only initialises the anchors
