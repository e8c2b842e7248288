"""GPU, two ranks on one card (gloo): the generators' EMA under data parallelism.  Replicas are bit-identical after every step and every rank runs the same
kernel on the same bits, so the twins and the counts are bit-identical across the ranks without a collective; one rank's inf reaches every rank's G measurement,
so every rank skips the three G steps AND the EMA update.  The ranks are fresh child processes; the parent waits with a limit, kills leftovers, never retries."""
import pytest

from tests import rig

pytestmark = pytest.mark.gpu


def _two_ranks(tmp_path, mode):
    return rig.run_ranks("ema_dp_worker.py", tmp_path, mode, tag=f"ema_{mode}", timeout=600)


def test_twins_and_counts_are_identical_across_ranks(tmp_path):
    a, b = _two_ranks(tmp_path, "plain")
    print(f"\n[ema dp] counts {a['counts']} / {b['counts']}, twin digests {[h[:8] for h in a['twin_sha']]}")
    assert a["twin_sha"] == b["twin_sha"] and a["live_sha"] == b["live_sha"]
    for r in (a, b):
        assert r["counts"] == [1, 2] and r["skipped_gen"] == [0.0, 0.0] and r["twin_forward_collectives"] == 0, r
        assert len(set(r["twin_sha"])) == 3 and r["twins_differ_from_live"], r      # start, after iteration 1, after iteration 2: the twin moved each time


def test_one_ranks_inf_skips_the_update_on_every_rank(tmp_path):
    a, b = _two_ranks(tmp_path, "inf")
    print(f"\n[ema dp, inf on rank 1] counts {a['counts']} / {b['counts']}, skipped {a['skipped_gen']} / {b['skipped_gen']}")
    assert a["twin_sha"] == b["twin_sha"] and a["live_sha"] == b["live_sha"]
    for r in (a, b):
        assert r["skipped_gen"] == [0.0, 1.0], r                                 # both ranks skip
        assert r["counts"] == [1, 1], r                                           # both counts stay
        assert r["twin_sha"][2] == r["twin_sha"][1] != r["twin_sha"][0], r      # both twins keep every bit — buffers included
        assert r["live_sha"][1] == r["live_sha"][0], r                            # (the skipped G steps moved no live parameter either)
