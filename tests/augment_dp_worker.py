"""Child process of tests/test_augment_dp_gpu.py: one data-parallel rank (gloo, cuda:0).
Leg "observe": a ClipAugment with interval 1; each rank observes its own hand-written logits, two boundaries; beside it one state block that observes the
concatenated logits through the C ABI without any collective.  Leg "step": the real DCVGAN modules at width / 8, trainer.StepRunner with
optim.DataParallelAdam and trainer.build_augment(adaptive, interval 2), different data and random streams on every rank, two iterations.
Usage: python tests/augment_dp_worker.py RANK WORLD PORT OUT.json"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

from tests import rig  # noqa: E402

NAN = float("nan")
LOGITS = [[[1.0, 2.0, -1.0, 0.0, NAN, 6.0], [3.0, 4.0, 5.0, 6.0, 7.0]],      # boundary 1: rank 0's (r = 2 / 6 alone), rank 1's (r = 1 alone); together 7 / 11
          [[-1.0, -2.0, 0.5], [-3.0, NAN, -0.0, -4.0]]]           # boundary 2
RULE = dict(p=0.3, target=0.6, interval=1, p_max=0.8, adjust_clips=16, batch=4)      # step = 4 * 1 / 16 = 0.25


def main():
    rank, world, port, out, _ = rig.rank_args()
    rig.init_rank(port, rank, world)
    from dcvgan_amd import augment, native, trainer
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    cfg = rig.small_cfg()
    res = {"rank": rank}

    # ---- leg "observe" ----
    aug = augment.ClipAugment(cfg, dev, adaptive=True, **RULE)
    assert aug.world == world and aug.pg is not None
    solo = augment.ClipAugment._host_state(RULE["p"], 0, 0, 0).to(dev)      # one process observing the concatenated logits: no collective
    L = native.lib()
    res["dp_state"], res["solo_state"] = [], []
    for it, per_rank in enumerate(LOGITS, start=1):
        aug.observe(torch.tensor(per_rank[rank], dtype=torch.float32, device=dev))
        aug.end_of_iteration(it)
        cat = torch.tensor([v for y in per_rank for v in y], dtype=torch.float32, device=dev)
        native.check(L.dcv_aug_observe(native.ptr(cat), cat.numel(), native.ptr(solo), native.stream_ptr()), "dcv_aug_observe")
        native.check(L.dcv_aug_adjust(native.ptr(solo), aug.target, aug.step, aug.p_max, native.stream_ptr()), "dcv_aug_adjust")
        res["dp_state"].append(aug.state_words())
        res["solo_state"].append([int(v) for v in solo.cpu().tolist()])
    res["observe_collectives"] = aug.collectives

    # ---- leg "step" ----
    models, _ = rig.seeded_models(cfg, dev, cfg.seed + 17 * rank, 1000 + cfg.seed + rank, broadcast=True)
    opts = trainer.build_optimizers(cfg, models, data_parallel=True)
    aug2 = trainer.build_augment(cfg, models, opts, p=0.5, adaptive=True, interval=2, adjust_clips=8, seed=1000 + rank)
    assert aug2.batch == cfg.batchsize * world
    xc, xg = rig.clip_pair(cfg, dev, cfg.seed + rank, geo_channels=1)
    runner = trainer.StepRunner(cfg, models, opts, trainer.build_loss(cfg), augment=aug2)

    sha = rig.sha_of

    def weights():
        return [p for n in trainer.MODEL_NAMES for p in models[n].parameters()]

    res["data_sha"] = sha([xc, xg])
    res["weights_sha"] = [sha(weights())]
    res["table_sha"] = sha([aug2.draw(2, 64, 64)])      # the ranks' draws differ through their seeds
    for it in range(2):
        runner.step(xc, xg, 3 + it)
        torch.cuda.synchronize()
        res["weights_sha"].append(sha(weights()))
    res["step_state"] = aug2.state_words()
    res["step_collectives"] = aug2.collectives
    res["finite"] = all(bool(torch.isfinite(t).all()) for t in weights())
    json.dump(res, open(out, "w"))
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
