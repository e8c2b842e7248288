"""Child process of tests/test_sync_bn_dp_gpu.py: one data-parallel rank with synchronised BatchNorm on cuda:0, gloo collectives (two ranks may share one card; RCCL
refuses that).  Usage: python tests/sync_bn_worker.py RANK WORLD PORT OUT.json MODE
MODE: "models-2+2" | "models-3+1": idis and vdis (width / 8, no input noise) on 4 real clips split over the ranks, against a one-process run on the 4 clips;
      "step" | "step-overlap" | "step-control": trainer.StepRunner over build_models(sync_bn=True) (control: False), distinct data and Philox streams per rank."""
import copy
import datetime
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

from tests import rig  # noqa: E402


def rel(a, b):
    a = a.detach().double().cpu(); b = b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def same_on_all_ranks(world, tensors) -> bool:
    """bit-identity of a list of tensors across the ranks"""
    mine = [t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes() if t.is_floating_point() else t.detach().cpu().numpy().tobytes() for t in tensors]
    every = [None] * world
    dist.all_gather_object(every, mine)
    return all(e == every[0] for e in every)


def models_mode(rank, world, split, dev, res):
    from dcvgan_amd import optim, trainer
    from dcvgan_amd.rng import PhiloxRng
    cfg = rig.small_cfg(use_noise=dict(idis=False, vdis=False, gdis=False))
    torch.manual_seed(cfg.seed)
    models = trainer.build_models(cfg, dev)
    models = {k: models[k] for k in ("idis", "vdis")}
    for m in models.values():
        optim.broadcast_module(m)
        m._rng = PhiloxRng(5)
        m.train()
    solo = copy.deepcopy(models)                               # the one-process twin: unmarked, runs all 4 clips
    group = optim.sync_batchnorm(models)
    assert group.world == world and group.rank == rank and optim.sync_bn_group_of(solo) is None
    xc, xg = rig.clip_pair(cfg, dev, 77, batch=4, geo_channels=1)
    lo = sum(split[:rank]); hi = lo + split[rank]
    bucket = optim.GradBucket()
    for m in models.values():
        bucket.add(m.parameters())

    def run(ms, a, b):
        """forward + backward of idis (frame 3) and vdis on clips a..b with the loss sum(y * cot[a:b]); -> outputs, input gradients"""
        ins = dict(idis=[xg[a:b, :, 3].contiguous().requires_grad_(True), xc[a:b, :, 3].contiguous().requires_grad_(True)],
                   vdis=[xg[a:b].clone().requires_grad_(True), xc[a:b].clone().requires_grad_(True)])
        ys, loss = {}, None
        for k in ("idis", "vdis"):
            y = ms[k](*ins[k]).reshape(b - a, -1)
            cot = torch.cos(torch.arange(4 * y.shape[1], dtype=torch.float32) * 0.37).view(4, -1)[a:b].to(dev)
            ys[k] = y.detach()
            t = (y * cot).sum()
            loss = t if loss is None else loss + t
        loss.backward()
        return ys, {k: [t.grad.detach() for t in v] for k, v in ins.items()}

    c0 = group.collectives
    ys, dins = run(models, lo, hi)
    res["sync_bn_collectives"] = group.collectives - c0
    bucket.reduce()                                            # the bucket's sum over the ranks
    ys_ref, dins_ref = run(solo, 0, 4)
    torch.cuda.synchronize()
    fig = {}
    for k in ("idis", "vdis"):
        fig[f"{k}.output"] = rel(ys[k], ys_ref[k][lo:hi])
        for name, t, r in zip(("xg", "xc"), dins[k], dins_ref[k]):
            fig[f"{k}.d{name}"] = rel(t, r[lo:hi])
        ref_p = dict(solo[k].named_parameters())
        for n, p in models[k].named_parameters():
            fig[f"{k}.grad.{n}"] = rel(p.grad, ref_p[n].grad)
        ref_b = dict(solo[k].named_buffers())
        for n, b in models[k].named_buffers():
            if b.is_floating_point():
                fig[f"{k}.buffer.{n}"] = rel(b, ref_b[n])
            else:
                res.setdefault("nbt_equal", True)
                res["nbt_equal"] = res["nbt_equal"] and bool(torch.equal(b, ref_b[n]))
    res["figures"] = fig
    res["worst"] = max(v for k, v in fig.items() if ".buffer." not in k)
    res["worst_buffer"] = max(v for k, v in fig.items() if ".buffer." in k)
    res["buffers_identical"] = same_on_all_ranks(world, [b for m in models.values() for b in m.buffers()])


def step_mode(rank, world, mode, dev, res):
    from dcvgan_amd import optim, trainer
    sync, overlap = mode != "step-control", mode == "step-overlap"
    cfg = rig.small_cfg()
    # deliberately different replicas, made identical by the broadcast; distinct noise / dropout / latent streams per rank
    models, _ = rig.seeded_models(cfg, dev, cfg.seed + 17 * rank, 1000 + rank, sync_bn=sync, broadcast=True)
    group = optim.sync_bn_group_of(models)
    assert (group is not None and group.world == world) if sync else group is None
    opts = trainer.build_optimizers(cfg, models, data_parallel=True, overlap=overlap)
    xc, xg = rig.clip_pair(cfg, dev, cfg.seed + rank, geo_channels=1)      # distinct data per rank
    runner = trainer.StepRunner(cfg, models, opts, trainer.build_loss(cfg))
    per_it, finite = [], True
    for it in range(2):
        c0 = group.collectives if sync else 0
        out = runner.step(xc, xg, 3 + it)
        per_it.append((group.collectives - c0) if sync else 0)
        finite = finite and all(bool(torch.isfinite(v).all()) for v in out.values())
    torch.cuda.synchronize()
    res["sync_bn_collectives_per_iteration"] = per_it
    res["losses_finite"] = finite
    res["params_identical"] = same_on_all_ranks(world, [p for m in models.values() for p in m.parameters()])
    res["buffers_identical"] = same_on_all_ranks(world, [b for m in models.values() for b in m.buffers()])
    res["running_stats_identical"] = same_on_all_ranks(world, [b for m in models.values() for b in m.buffers() if b.is_floating_point()])
    if overlap:
        res["early_collectives"] = sum(b.early for b in {id(o.bucket): o.bucket for o in opts.values()}.values())


def main():
    rank, world, port, out, (mode,) = rig.rank_args()
    rig.init_rank(port, rank, world, timeout=datetime.timedelta(seconds=120))
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    res = {"rank": rank, "mode": mode}
    if mode.startswith("models-"):
        models_mode(rank, world, tuple(int(v) for v in mode[7:].split("+")), dev, res)
    else:
        step_mode(rank, world, mode, dev, res)
    json.dump(res, open(out, "w"))
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
