"""GPU, two ranks on one card (gloo): the device-resident dataset under data parallelism.  Each rank's ClipSampler takes its rank and world from torch.distributed
and computes its own slice of the epoch — no sampler object shared, no communication; the rank's batch is its slice of the single-process batch of size 2 B, byte
for byte, across an epoch boundary.  The only collective calls are the check's own (tests/clipstore_dp_worker.py).  The two ranks are fresh child processes, started
once for this module; the parent waits for each with a limit, kills leftovers, never retries."""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def ranks(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("clipstore_dp")
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    outs = [str(tmp / f"clipstore{r}.json") for r in range(2)]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "clipstore_dp_worker.py"), str(r), "2", str(port), outs[r]], env=env) for r in range(2)]
    try:
        for p in procs:
            assert p.wait(timeout=300) == 0
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    return [json.load(open(o)) for o in outs]


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
