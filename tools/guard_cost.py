"""What the gradient guard costs: isogd-depth in fp32 at B = 70 (or argv[1]), one process, 10 warm-up iterations, then three alternating pairs of 20 iterations
with the guard off and on (two runners over two copies of the models, the same data), timed with device events around each leg.
Usage: python tools/guard_cost.py [B] [out.txt]      (the record also goes to stdout)"""
import copy
import sys
sys.path.insert(0, '.')
import torch
from dcvgan_amd import native, trainer
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
runners = {"off": trainer.StepRunner(cfg, models["off"], trainer.build_optimizers(cfg, models["off"]), trainer.build_loss(cfg)),
           "on": trainer.StepRunner(cfg, models["on"], trainer.build_optimizers(cfg, models["on"], guard=dict(max_norm=1e3)), trainer.build_loss(cfg))}
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
lines = ["guard cost: isogd-depth fp32, B = %d, %d warm-up iterations per arm, %d alternating pairs of %d iterations, device events; library %s" % (B, WARM, PAIRS, LEG, native.csrc_digest()[:12])]
ms = {"off": [], "on": []}
for p in range(PAIRS):
    row = {}
    for arm in ("off", "on"):
        t, launches, out = leg(arm, LEG)
        ms[arm].append(t); row[arm] = (t, launches)
    lines.append("pair %d: guard off %.2f ms / iteration (%.0f library launches) | guard on %.2f ms (%.0f launches) | difference %+.2f ms" %
                 (p + 1, row["off"][0], row["off"][1], row["on"][0], row["on"][1], row["on"][0] - row["off"][0]))
mean = {a: sum(v) / len(v) for a, v in ms.items()}
n_grad = sum(p.numel() for m in models["on"].values() for p in m.parameters())
lines.append("mean: off %.2f ms, on %.2f ms, guard %+.2f ms (%+.2f %%); spread of the guard-off legs %.2f ms; gradients read once more: %.1f MB" %
             (mean["off"], mean["on"], mean["on"] - mean["off"], 100.0 * (mean["on"] - mean["off"]) / mean["off"], max(ms["off"]) - min(ms["off"]), n_grad * 4 / 1e6))
lines.append("last iteration with the guard: " + ", ".join("%s %.4g" % (k, float(v)) for k, v in sorted(out.items())))
print("\n".join(lines))
if OUT:
    open(OUT, "w").write("\n".join(lines) + "\n")
