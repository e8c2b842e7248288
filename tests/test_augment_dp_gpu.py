"""GPU, two ranks on one card (gloo): the augmentation's adaptive probability under data parallelism.  Before every adjustment the two accumulators are
all-reduced (SUM, int32: exact and order-free) over the feature's own process group, so every rank holds the same p — the p of one process that observed the
concatenated logits — and the replicas stay bit-identical, as they are without the feature.  The two ranks are fresh child processes, started once for this
module; the parent waits for each with a limit, kills leftovers, never retries."""
import pytest

from tests import rig
from tests import test_augment_cpu as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ranks(tmp_path_factory):
    return rig.run_ranks("augment_dp_worker.py", tmp_path_factory.mktemp("augment_dp"), tag="aug", timeout=300)


def test_every_rank_holds_the_p_of_one_process_on_the_concatenated_logits(ranks):
    from tests.augment_dp_worker import LOGITS, RULE
    a, b = ranks
    step = RULE["batch"] * RULE["interval"] / RULE["adjust_clips"]
    want, state = [], [R.f32_bits(RULE["p"]), 0, 0, 0, 0, 0, 0, 0]
    for per_rank in LOGITS:
        for y in per_rank:
            state = R.observe_ref(state, y)
        state = R.adjust_ref(state, RULE["target"], step, RULE["p_max"])
        want.append(state)
    ps = [float(R.bits_f32(s[0])) for s in a["dp_state"]]
    print(f"\n[augment dp] p after the two boundaries {ps}; states {a['dp_state']}")
    assert a["dp_state"] == b["dp_state"] == a["solo_state"] == b["solo_state"] == want
    for s in a["dp_state"]:
        assert s[1] == 0 and s[2] == 0                      # the accumulators are zeroed on both ranks
    assert [s[3] for s in a["dp_state"]] == [1, 2] and a["observe_collectives"] == b["observe_collectives"] == 2
    assert ps[0] > RULE["p"] and ps[1] < ps[0]              # up on the first boundary (r = 7 / 11; rank 0 alone would have gone down), down on the second (r = -3 / 7)


def test_replicas_stay_bit_identical_in_the_iteration(ranks):
    a, b = ranks
    print(f"\n[augment dp step] weights {[h[:8] for h in a['weights_sha']]}, state {a['step_state']}")
    assert a["data_sha"] != b["data_sha"] and a["table_sha"] != b["table_sha"]      # distinct data, distinct draws
    assert a["weights_sha"] == b["weights_sha"] and len(set(a["weights_sha"])) == 3
    assert a["step_state"] == b["step_state"] and a["step_state"][3] == 1 and a["step_state"][1:3] == [0, 0]
    assert a["step_collectives"] == b["step_collectives"] == 1 and a["finite"] and b["finite"]
