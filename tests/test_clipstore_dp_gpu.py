"""GPU, two ranks on one card (gloo): the device-resident dataset under data parallelism.  Each rank's ClipSampler takes its rank and world from torch.distributed
and computes its own slice of the epoch — no sampler object shared, no communication; the rank's batch is its slice of the single-process batch of size 2 B, byte
for byte, across an epoch boundary.  The only collective calls are the check's own (tests/clipstore_dp_worker.py).  The two ranks are fresh child processes, started
once for this module; the parent waits for each with a limit, kills leftovers, never retries."""
import pytest

from tests import rig

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ranks(tmp_path_factory):
    return rig.run_ranks("clipstore_dp_worker.py", tmp_path_factory.mktemp("clipstore_dp"), tag="clipstore", timeout=300)


def test_each_rank_reads_its_slice_of_the_single_process_batch(ranks):
    from tests.clipstore_dp_worker import ITERATIONS
    a, b = ranks
    print(f"\n[clipstore dp] states {a['state']}; batch hashes {[h[:8] for h in a['sha']]} / {[h[:8] for h in b['sha']]}")
    for r, res in enumerate(ranks):
        assert (res["sampler_rank"], res["sampler_world"]) == (r, 2) and res["len"] == [2, 2]
        assert res["slice_equal"] == res["table_equal"] == res["gathered_equal"] == [True] * ITERATIONS, res
        assert res["state"] == [[0, 1], [1, 0], [1, 1], [2, 0], [2, 1]]      # two iterations per epoch: the batches cross two epoch boundaries
    assert all(x != y for x, y in zip(a["sha"], b["sha"]))                   # the ranks hold different clips
    assert len(set(a["sha"])) == ITERATIONS                                  # and every batch is another one
