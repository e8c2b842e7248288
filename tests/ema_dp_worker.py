"""Child process of tests/test_ema_dp_gpu.py: one data-parallel rank (the real DCVGAN modules at width / 8, trainer.StepRunner, optim.DataParallelAdam with a
GradGuard per phase, synchronised BatchNorm, trainer.build_ema; gloo, cuda:0), different data and random streams on every rank, two iterations.  BatchNorm is
synchronised because the twins carry copies of the running statistics: with distinct data per rank those are the same on every rank only when the statistics
cover every rank's batch (tests/test_sync_bn_dp_gpu.py has the control) — the parameters are identical either way.  Mode "inf": rank 1 writes one inf into a
local generator gradient right before the second iteration's G-phase measurement.  Usage: python tests/ema_dp_worker.py RANK WORLD PORT OUT.json plain|inf"""
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
    from dcvgan_amd import optim, trainer
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    cfg = rig.small_cfg()
    models, _ = rig.seeded_models(cfg, dev, cfg.seed + 17 * rank, 1000 + cfg.seed + rank, sync_bn=True, broadcast=True)
    opts = trainer.build_optimizers(cfg, models, data_parallel=True, guard=dict(max_norm=10.0))
    guard_g = opts["ggen"].guard
    ema = trainer.build_ema(cfg, models, opts, decay=0.9)
    assert ema.guard is guard_g and guard_g is not None and ema.guard is not opts["idis"].guard
    group = optim.sync_bn_group_of(models)
    assert group is not None and group.world == world and optim.sync_bn_group_of(ema.twins) is group      # the twins carry the mark ...
    xc, xg = rig.clip_pair(cfg, dev, cfg.seed + rank, geo_channels=1)
    runner = trainer.StepRunner(cfg, models, opts, trainer.build_loss(cfg), ema=ema)

    orig = guard_g.measure

    def measure():
        if mode == "inf" and runner.iteration == 2 and rank == 1:
            victim = next(p for p in models["cgen"].parameters() if p.grad is not None and p.numel() > 100)
            victim.grad.view(-1)[37] = float("inf")      # a LOCAL gradient, before the reduction: the all-reduce carries it to every rank
        orig()
    guard_g.measure = measure

    def twins():
        return [v for n in ema.names for v in ema.module(n).state_dict().values()]

    def live():
        return [p for n in ema.names for p in models[n].parameters()]

    res = {"rank": rank, "mode": mode, "twin_sha": [rig.sha_of(twins())], "live_sha": [], "counts": [], "skipped_gen": []}
    for it in range(2):
        o = runner.step(xc, xg, 3 + it)
        torch.cuda.synchronize()
        res["twin_sha"].append(rig.sha_of(twins()))
        res["live_sha"].append(rig.sha_of(live()))
        res["counts"].append(ema.num_updates())
        res["skipped_gen"].append(float(o["skipped_gen"]))
    from dcvgan_amd import sampling
    c0 = group.collectives
    sampling.generate_samples(ema.module("ggen"), ema.module("cgen"), num=2, batchsize=2)
    res["twin_forward_collectives"] = group.collectives - c0      # ... and, in eval mode, never exchange
    first_64k = lambda ts: torch.cat([rig.byte_view(t) for t in ts])[:1 << 16]
    res["twins_differ_from_live"] = not torch.equal(first_64k(twins()), first_64k(v for n in ema.names for v in models[n].state_dict().values()))
    json.dump(res, open(out, "w"))
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
