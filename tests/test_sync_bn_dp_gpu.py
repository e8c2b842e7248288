"""GPU, two ranks on one card (gloo): synchronised BatchNorm (optim.sync_batchnorm) over the real DCVGAN modules.
The ranks are fresh child processes (tests/sync_bn_worker.py; never a re-exec of this one); the parent waits with a limit, kills leftovers and never retries.

Bars (tests/test_ops_gpu.py::test_bn_act's): rel() < 1e-3 on outputs and gradients, < 1e-5 on the running statistics."""
import pytest

from tests import rig

pytestmark = pytest.mark.gpu
TOL, TOL_STATS = 1e-3, 1e-5


def _run(mode, tmp_path):
    return rig.run_ranks("sync_bn_worker.py", tmp_path, mode, tag=mode, timeout=300)


@pytest.mark.parametrize("split", ["2+2", "3+1"])
def test_two_ranks_equal_one_process_on_the_whole_batch(tmp_path, split):
    """idis and vdis at width / 8 without input noise, 4 real clips split over two ranks with per-rank losses L_r: the bucket-summed parameter gradients, the input
    gradients, the outputs and the BatchNorm buffers are those of ONE process that runs the 4 clips with the loss L_0 + L_1, and the buffers are
    bit-identical across the ranks."""
    res = _run("models-" + split, tmp_path)
    for r in res:
        worst = sorted(r["figures"].items(), key=lambda kv: -kv[1])[:3]
        print(f"sync-bn two ranks {split} rank {r['rank']}: outputs/gradients {r['worst']:.3g}, running statistics {r['worst_buffer']:.3g}, "
              f"{r['sync_bn_collectives']} collectives; largest: {worst}")
    for r in res:
        assert r["sync_bn_collectives"] == res[0]["sync_bn_collectives"] > 0, r      # one per BatchNorm group and pass, alike on both ranks
        assert r["worst"] < TOL, r
        assert r["worst_buffer"] < TOL_STATS and r["nbt_equal"], r
        assert r["buffers_identical"], r


@pytest.mark.parametrize("mode", ["step", "step-overlap"])
def test_step_runner_keeps_the_replicas_and_their_statistics_identical(tmp_path, mode):
    """trainer.StepRunner over build_models(sync_bn=True), distinct data and Philox streams per rank, two iterations, plain and overlapped gradient reduction:
    parameters AND every BatchNorm buffer are bit-identical across the ranks (broadcast_buffers has nothing left to patch), the losses are finite, and both ranks
    issue the same number of sync-BN collectives per iteration."""
    res = _run(mode, tmp_path)
    print(f"sync-bn {mode}: collectives per iteration {res[0]['sync_bn_collectives_per_iteration']}")
    for r in res:
        assert r["losses_finite"], r
        assert r["params_identical"] and r["buffers_identical"], r
        assert r["sync_bn_collectives_per_iteration"] == res[0]["sync_bn_collectives_per_iteration"], res
        assert r["sync_bn_collectives_per_iteration"][0] == r["sync_bn_collectives_per_iteration"][1] > 0, r


def test_without_sync_bn_the_running_statistics_differ(tmp_path):
    """The control: the same two ranks with sync_bn=False keep identical parameters but NOT identical running statistics — the difference the test above must see."""
    for r in _run("step-control", tmp_path):
        assert r["losses_finite"] and r["params_identical"], r
        assert not r["running_stats_identical"] and not r["buffers_identical"], r
