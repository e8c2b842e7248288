"""Child process of tests/test_spectral_dp_gpu.py: one data-parallel rank (the real DCVGAN modules at width / 8, trainer.StepRunner, optim.DataParallelAdam with a
GradGuard per phase, trainer.build_spectral_norm; gloo, cuda:0), different data and random streams on every rank, two iterations.  Mode "overlap": the buckets'
collectives start during the backward.  Mode "inf": rank 1 writes one inf into a local discriminator gradient right before the second iteration's projection.
Usage: python tests/spectral_dp_worker.py RANK WORLD PORT OUT.json plain|overlap|inf"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

from tests import rig  # noqa: E402


def main():
    rank, world, port, out, (mode,) = rig.rank_args()
    rig.init_rank(port, rank, world)
    from dcvgan_amd import trainer
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    cfg = rig.small_cfg()
    models, _ = rig.seeded_models(cfg, dev, cfg.seed + 17 * rank, 1000 + cfg.seed + rank, broadcast=True)
    opts = trainer.build_optimizers(cfg, models, data_parallel=True, overlap=(mode == "overlap"), guard=dict(max_norm=10.0))
    sn = trainer.build_spectral_norm(cfg, models, opts)      # the same seed on every rank
    guard_d = opts["idis"].guard
    assert sn.guard is guard_d and guard_d is not None and len(sn._dp) == 3 and len(sn.convs) == 14
    xc, xg = rig.clip_pair(cfg, dev, cfg.seed + rank, geo_channels=1)
    runner = trainer.StepRunner(cfg, models, opts, trainer.build_loss(cfg), spectral=sn)

    orig = sn.project

    def project():
        if mode == "inf" and runner.iteration == 2 and rank == 1:
            victim = next(c.weight for c in sn.convs if c.weight.grad is not None and c.weight.numel() > 100)
            victim.grad.view(-1)[37] = float("inf")      # a LOCAL gradient, before the reduction: the all-reduce carries it to every rank
        orig()
    sn.project = project

    sha = rig.sha_of

    def weights():
        return [p for n in ("idis", "vdis", "gdis") for p in models[n].parameters()]

    def spectral():
        return [t for c in sn.convs for t in (c.weight_u, c.weight_v, c.weight_sigma, c.__dict__["_dcv_spectral"].w_sn)]

    res = {"rank": rank, "mode": mode, "weights_sha": [sha(weights())], "spectral_sha": [sha(spectral())], "skipped_dis": [], "data_sha": sha([xc, xg]),
           "reductions": None, "early": None}
    for it in range(2):
        o = runner.step(xc, xg, 3 + it)
        torch.cuda.synchronize()
        res["weights_sha"].append(sha(weights()))
        res["spectral_sha"].append(sha(spectral()))
        res["skipped_dis"].append(float(o["skipped_dis"]))
    res["reductions"], res["early"] = opts["idis"].bucket.reductions, opts["idis"].bucket.early
    res["finite"] = all(bool(torch.isfinite(t).all()) for t in spectral() + weights())
    json.dump(res, open(out, "w"))
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
