"""What synchronised BatchNorm costs on one card: isogd-depth in fp32 at B = 70 (or argv[1]), one process, 10 warm-up iterations, then three alternating pairs of 20
iterations with the models unmarked and marked with optim.sync_batchnorm(force=True) — the sync kernels at world 1, no collective (two runners over two copies
of the models, the same data), timed with device events around each leg.  The collective's own time at N > 1 is not part of this number.
Usage: python tools/sync_bn_cost.py [B] [out.txt]      (the record also goes to stdout)"""
import copy
import sys
sys.path.insert(0, '.')
import torch
from dcvgan_amd import native, optim, trainer
from dcvgan_amd.configs import CONFIGS

B = int(sys.argv[1]) if len(sys.argv) > 1 else 70
OUT = sys.argv[2] if len(sys.argv) > 2 else None
WARM, LEG, PAIRS = 10, 20, 3
native.lib()
dev = torch.device("cuda:0")
cfg = CONFIGS["isogd-depth"].scaled(batchsize=B)
torch.manual_seed(1)
models = {"off": trainer.build_models(cfg, dev)}
models["on"] = copy.deepcopy(models["off"])
group = optim.sync_batchnorm(models["on"], force=True)
runners = {arm: trainer.StepRunner(cfg, models[arm], trainer.build_optimizers(cfg, models[arm]), trainer.build_loss(cfg)) for arm in ("off", "on")}
g = torch.Generator().manual_seed(2)
xc = (torch.rand(B, 3, 16, 64, 64, generator=g) * 2 - 1).to(dev); xg = (torch.rand(B, cfg.channel, 16, 64, 64, generator=g) * 2 - 1).to(dev)


def leg(arm, n):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    c0 = native.launch_count()
    e0.record()
    for i in range(n):
        out = runners[arm].step(xc, xg, i % 16)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n, (native.launch_count() - c0) / n, out


for arm in ("off", "on"):
    leg(arm, WARM)
lines = ["sync-BN cost: isogd-depth fp32, B = %d, world 1 (force: sync kernels, no collective), %d warm-up iterations per arm, %d alternating pairs of %d iterations, "
         "device events; library %s" % (B, WARM, PAIRS, LEG, native.csrc_digest()[:12])]
ms = {"off": [], "on": []}
launches = {}
for p in range(PAIRS):
    row = {}
    for arm in ("off", "on"):
        t, n_launch, out = leg(arm, LEG)
        ms[arm].append(t); row[arm] = (t, n_launch); launches[arm] = n_launch
    lines.append("pair %d: unmarked %.2f ms / iteration (%.0f library launches) | sync-BN %.2f ms (%.0f launches) | difference %+.2f ms" %
                 (p + 1, row["off"][0], row["off"][1], row["on"][0], row["on"][1], row["on"][0] - row["off"][0]))
mean = {a: sum(v) / len(v) for a, v in ms.items()}
lines.append("mean: unmarked %.2f ms, sync-BN %.2f ms, difference %+.2f ms (%+.2f %%); spread of the unmarked legs %.2f ms; library launches per iteration %+.0f" %
             (mean["off"], mean["on"], mean["on"] - mean["off"], 100.0 * (mean["on"] - mean["off"]) / mean["off"], max(ms["off"]) - min(ms["off"]),
              launches["on"] - launches["off"]))
lines.append("last iteration with sync-BN: " + ", ".join("%s %.4g" % (k, float(v)) for k, v in sorted(out.items())) + "; collectives %d" % group.collectives)
print("\n".join(lines))
if OUT:
    open(OUT, "w").write("\n".join(lines) + "\n")
