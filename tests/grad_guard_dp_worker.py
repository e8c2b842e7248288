"""Child process of tests/test_grad_guard_dp_gpu.py: one data-parallel rank (the real DCVGAN modules at width / 8, trainer.StepRunner, optim.DataParallelAdam,
gloo, cuda:0) with a GradGuard per phase, different data on every rank, three iterations.  Rank 1 writes one inf into a local generator gradient right before the
second iteration's G-phase measurement.  Usage: python tests/grad_guard_dp_worker.py RANK WORLD PORT OUT.json"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

from tests import rig  # noqa: E402


def main():
    rank, world, port, out, _ = rig.rank_args()
    rig.init_rank(port, rank, world)
    from dcvgan_amd import trainer
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    cfg = rig.small_cfg()
    models, _ = rig.seeded_models(cfg, dev, cfg.seed + 17 * rank, 1000 + cfg.seed + rank, broadcast=True)
    opts = trainer.build_optimizers(cfg, models, data_parallel=True, guard={})
    guard_d, guard_g = opts["idis"].guard, opts["ggen"].guard
    assert opts["cgen"].guard is guard_g and opts["gdis"].guard is guard_d and guard_d is not guard_g
    xc, xg = rig.clip_pair(cfg, dev, cfg.seed + rank, geo_channels=1)
    runner = trainer.StepRunner(cfg, models, opts, trainer.build_loss(cfg))

    orig = guard_g.measure

    def measure():
        if runner.iteration == 2 and rank == 1:
            victim = next(p for p in models["cgen"].parameters() if p.grad is not None and p.numel() > 100)
            victim.grad.view(-1)[37] = float("inf")      # a LOCAL gradient, before the reduction: the all-reduce carries it to every rank
        orig()
    guard_g.measure = measure

    def gen_params():
        return torch.cat([p.detach().reshape(-1) for n in ("ggen", "cgen") for p in models[n].parameters()]).cpu()

    def dis_params():
        return torch.cat([p.detach().reshape(-1) for n in ("idis", "vdis", "gdis") for p in models[n].parameters()]).cpu()

    bits = lambda t: int(t.detach().cpu().view(torch.int32).item())
    res = {"rank": rank, "norm_bits": [], "skipped": [], "gen_moved": [], "dis_moved": []}
    for it in range(3):
        g0, d0 = gen_params(), dis_params()
        o = runner.step(xc, xg, 3 + it)
        torch.cuda.synchronize()
        res["norm_bits"].append([bits(o["grad_norm_dis"]), bits(o["grad_norm_gen"])])
        res["skipped"].append([float(o["skipped_dis"]), float(o["skipped_gen"])])
        res["gen_moved"].append(float((gen_params() != g0).float().mean()))
        res["dis_moved"].append(float((dis_params() != d0).float().mean()))
    res["skipped_total"] = [float(guard_d.stats()["skipped_total"]), float(guard_g.stats()["skipped_total"])]
    res["grad_scale"] = [o.inner.grad_scale for o in opts.values()]
    res["gen_steps"] = sorted({int(s["step"].item()) for s in opts["ggen"].inner.state.values()}), sorted({int(s["step"].item()) for s in opts["cgen"].inner.state.values()})
    params = torch.cat([gen_params(), dis_params()])
    allp = [None] * world
    dist.all_gather_object(allp, params.numpy())
    res["replicas_identical"] = bool(all((a == allp[0]).all() for a in allp))
    json.dump(res, open(out, "w"))
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
