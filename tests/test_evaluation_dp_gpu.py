"""GPU, two ranks on one card (gloo): the evaluation statistics under data parallelism.  The states are additive, so after all_reduce (SUM over sum, gram, the
Inception sums and the row counts) every rank holds the state of one process that saw all the rows: exactly for the moments of integer-valued features, and to the
Inception sums' bar for the rest.  The two ranks are fresh child processes, started once for this module; the parent waits for each with a limit, kills leftovers,
never retries."""
import numpy as np
import pytest

from tests import rig
from tests import test_evaluation_cpu as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ranks(tmp_path_factory):
    return rig.run_ranks("evaluation_dp_worker.py", tmp_path_factory.mktemp("evaluation_dp"), tag="evaluation", timeout=300)


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
