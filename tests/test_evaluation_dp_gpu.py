"""GPU, two ranks on one card (gloo): the evaluation statistics under data parallelism.  The states are additive, so after all_reduce (SUM over sum, gram, the
Inception sums and the row counts) every rank holds the state of one process that saw all the rows: exactly for the moments of integer-valued features, and to the
Inception sums' bar for the rest.  The two ranks are fresh child processes, started once for this module; the parent waits for each with a limit, kills leftovers,
never retries."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from tests import test_evaluation_cpu as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def ranks(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("evaluation_dp")
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    outs = [str(tmp / f"evaluation{r}.json") for r in range(2)]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "evaluation_dp_worker.py"), str(r), "2", str(port), outs[r]], env=env) for r in range(2)]
    try:
        for p in procs:
            assert p.wait(timeout=300) == 0
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    return [json.load(open(o)) for o in outs]


def test_every_rank_holds_the_single_process_state(ranks):
    from dcvgan_amd import evaluation as E
    from tests.evaluation_dp_worker import CLASSES, N_ROWS, data, rows_of
    a, b = ranks
    feats, logits = data()
    assert a["n_before"] == [rows_of(0, 2).stop - rows_of(0, 2).start] * 2 and b["n_before"] == [N_ROWS - a["n_before"][0]] * 2 and a["n_before"] != b["n_before"]
    xi = feats.astype(np.int64)
    for r in (a, b):
        assert r["n"] == [N_ROWS, N_ROWS]
        assert np.array_equal(np.array(r["sum"]), xi.sum(0).astype(np.float64))                 # the moments: exactly the single-process state
        assert np.array_equal(np.array(r["gram"]), (xi.T @ xi).astype(np.float64))
    assert a["inception"] == b["inception"] and a["score"] == b["score"]
    got, want = np.array(a["inception"]), R.inception_ref(logits)
    bar = 4 * N_ROWS * CLASSES * R.EPS
    rel = np.abs(got - want) / np.abs(want)
    print(f"\n[evaluation dp] Inception sums: worst relative difference {rel.max():.3g}, bar {bar:.3g}; score {a['score']!r}")
    assert np.all(rel <= bar)
    assert abs(a["score"] - E.inception_score_from_state(want, N_ROWS)) <= 4 * bar * np.log(CLASSES) * a["score"]
