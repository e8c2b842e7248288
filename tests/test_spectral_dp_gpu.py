"""GPU, two ranks on one card (gloo): spectral normalisation under data parallelism.  The projection acts on the reduced gradient and every rank runs the same
kernels on the same bits, so the weights, u, v, sigma and W / sigma are bit-identical across the ranks without a collective of their own — with plain buckets and
with collectives overlapped with the backward; one rank's inf reaches every rank's D measurement, so every rank skips the three D steps AND the power iteration.
The ranks are fresh child processes; the parent waits with a limit, kills leftovers, never retries."""
import pytest

from tests import rig

pytestmark = pytest.mark.gpu


def _two_ranks(tmp_path, mode):
    return rig.run_ranks("spectral_dp_worker.py", tmp_path, mode, tag=f"sn_{mode}", timeout=600)


@pytest.mark.parametrize("mode", ["plain", "overlap"])
def test_replicas_stay_bit_identical(tmp_path, mode):
    a, b = _two_ranks(tmp_path, mode)
    print(f"\n[spectral dp, {mode}] weights {[h[:8] for h in a['weights_sha']]}, u/v/sigma/W_sn {[h[:8] for h in a['spectral_sha']]}, early collectives {a['early']}")
    assert a["data_sha"] != b["data_sha"]                                            # distinct data
    assert a["weights_sha"] == b["weights_sha"] and a["spectral_sha"] == b["spectral_sha"]
    for r in (a, b):
        assert r["skipped_dis"] == [0.0, 0.0] and r["finite"] and r["reductions"] >= 2, r
        assert len(set(r["weights_sha"])) == 3 and len(set(r["spectral_sha"])) == 3, r      # start, iteration 1, iteration 2: both moved each time
    if mode == "overlap":
        assert a["early"] > 0 and b["early"] > 0


def test_one_ranks_inf_skips_the_update_on_every_rank(tmp_path):
    a, b = _two_ranks(tmp_path, "inf")
    print(f"\n[spectral dp, inf on rank 1] skipped {a['skipped_dis']} / {b['skipped_dis']}")
    assert a["weights_sha"] == b["weights_sha"] and a["spectral_sha"] == b["spectral_sha"]
    for r in (a, b):
        assert r["skipped_dis"] == [0.0, 1.0] and r["finite"], r                     # both ranks skip
        assert r["weights_sha"][2] == r["weights_sha"][1] != r["weights_sha"][0], r    # no discriminator weight moved ...
        assert r["spectral_sha"][2] == r["spectral_sha"][1] != r["spectral_sha"][0], r      # ... and no bit of u, v, sigma or W / sigma
