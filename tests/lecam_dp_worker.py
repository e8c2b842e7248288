"""Child process of tests/test_lecam_dp_gpu.py: one data-parallel rank (gloo, cuda:0).
Leg "anchors": a LeCam over three discriminators; each rank hands it its own logits (multiples of 2^-8 below 8 in magnitude: every sum is exact, in any order), three
iterations.  Leg "step": the real DCVGAN modules at width / 8, trainer.StepRunner with optim.DataParallelAdam and trainer.build_lecam(start=0), different data and
random streams on every rank, two iterations.
Usage: python tests/lecam_dp_worker.py RANK WORLD PORT OUT.json"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from tests import rig  # noqa: E402

SIZES = [(2, 2), (128, 128), (300, 77)]      # (real, fake) logits per rank of the three discriminators
RULE = dict(weight=0.3, decay=0.9, start=0, one_sided=True)
ITERATIONS = 3


def logits(iteration, rank):
    """-> (y_reals, y_fakes) of `rank` in `iteration`: fp32 multiples of 2^-8, |y| < 8."""
    g = np.random.default_rng(1000 + 10 * iteration + rank)
    draw = lambda n: (g.integers(-2047, 2048, size=n).astype(np.float64) / 256.0).astype(np.float32)
    return [draw(a) for a, _ in SIZES], [draw(b) for _, b in SIZES]


def main():
    import torch
    import torch.distributed as dist
    rank, world, port, out, _ = rig.rank_args()
    rig.init_rank(port, rank, world)
    from dcvgan_amd import lecam, loss, trainer
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    cfg = rig.small_cfg()
    res = {"rank": rank}

    # ---- leg "anchors" ----
    lc = lecam.LeCam(3, device=dev, **RULE)
    assert lc.world == world and lc.pg is not None
    hinge = loss.HingeLoss()
    res["states"], res["regs"] = [], []
    for it in range(ITERATIONS):
        yr, yf = logits(it, rank)
        lc.compute_dis_losses(hinge, [torch.from_numpy(y).to(dev) for y in yr], [torch.from_numpy(y).to(dev) for y in yf])
        res["states"].append(lc.state_words())
        res["regs"].append([float(v) for v in lc.reg.cpu().tolist()])
    res["anchor_collectives"] = lc.collectives

    # ---- leg "step" ----
    models, _ = rig.seeded_models(cfg, dev, cfg.seed + 17 * rank, 1000 + cfg.seed + rank, broadcast=True)
    opts = trainer.build_optimizers(cfg, models, data_parallel=True)
    lc2 = trainer.build_lecam(cfg, models, opts, weight=0.3, start=0)
    xc, xg = rig.clip_pair(cfg, dev, cfg.seed + rank, geo_channels=1)
    runner = trainer.StepRunner(cfg, models, opts, trainer.build_loss(cfg), lecam=lc2)

    sha = rig.sha_of

    def weights():
        return [p for n in trainer.MODEL_NAMES for p in models[n].parameters()]

    res["data_sha"] = sha([xc, xg])
    res["weights_sha"] = [sha(weights())]
    res["step_regs"] = []
    for it in range(2):
        o = runner.step(xc, xg, 3 + it)
        torch.cuda.synchronize()
        res["weights_sha"].append(sha(weights()))
        res["step_regs"].append([float(o[k]) for k in ("lecam_idis", "lecam_vdis", "lecam_gdis")])
    res["step_state"] = lc2.state_words()
    res["step_collectives"] = lc2.collectives
    res["finite"] = all(bool(torch.isfinite(t).all()) for t in weights())
    json.dump(res, open(out, "w"))
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
