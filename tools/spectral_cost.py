"""What spectral normalisation of the discriminators costs: isogd-depth in fp32 at B = 70 (or argv[1]), 10 warm-up iterations per arm, then three alternating pairs of 20
iterations with it off and on (two runners over two copies of the models, the same data), timed with device events around each leg.  The "on" arm trains other
weights (W / sigma), so only the time and the launch count are compared, not the losses.  The measuring leg is a fresh child process under its own time limit; a
failure ends the script there.
Usage: python tools/spectral_cost.py [B] [out.txt]      (default out: profiles/spectral_cost.txt; the record also goes to stdout)"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARM, LEG, PAIRS = 10, 20, 3
LIMIT_S = 420


def measure(B, out):
    import copy
    import torch
    from dcvgan_amd import native, trainer
    from dcvgan_amd.configs import CONFIGS
    native.lib()
    dev = torch.device("cuda:0")
    cfg = CONFIGS["isogd-depth"].scaled(batchsize=B)
    torch.manual_seed(1)
    models = {"off": trainer.build_models(cfg, dev)}
    models["on"] = copy.deepcopy(models["off"])
    opts = {a: trainer.build_optimizers(cfg, models[a]) for a in ("off", "on")}
    sn = trainer.build_spectral_norm(cfg, models["on"], opts["on"])
    runners = {"off": trainer.StepRunner(cfg, models["off"], opts["off"], trainer.build_loss(cfg)),
               "on": trainer.StepRunner(cfg, models["on"], opts["on"], trainer.build_loss(cfg), spectral=sn)}
    g = torch.Generator().manual_seed(2)
    xc = (torch.rand(B, 3, 16, 64, 64, generator=g) * 2 - 1).to(dev); xg = (torch.rand(B, cfg.channel, 16, 64, 64, generator=g) * 2 - 1).to(dev)

    def leg(arm, n):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        c0 = native.launch_count()
        e0.record()
        for i in range(n):
            runners[arm].step(xc, xg, i % 16)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n, (native.launch_count() - c0) / n

    for arm in ("off", "on"):
        leg(arm, WARM)
    lines = ["spectral normalisation cost: isogd-depth fp32, B = %d, %d warm-up iterations per arm, %d alternating pairs of %d iterations, device events; library %s" %
             (B, WARM, PAIRS, LEG, native.csrc_digest()[:12])]
    ms, diffs = {"off": [], "on": []}, []
    for p in range(PAIRS):
        row = {}
        for arm in ("off", "on"):
            row[arm] = leg(arm, LEG)
            ms[arm].append(row[arm][0])
        diffs.append(row["on"][0] - row["off"][0])
        lines.append("pair %d: off %.2f ms / iteration (%.0f library launches) | on %.2f ms (%.0f launches) | difference %+.3f ms" %
                     (p + 1, row["off"][0], row["off"][1], row["on"][0], row["on"][1], diffs[-1]))
    mean = {a: sum(v) / len(v) for a, v in ms.items()}
    n_w = sum(c.weight.numel() for c in sn.convs)
    lines.append("mean: off %.2f ms, on %.2f ms, spectral normalisation %+.3f ms (%+.2f %%); spread of the pairs' differences %.3f ms, of the off legs %.2f ms" %
                 (mean["off"], mean["on"], mean["on"] - mean["off"], 100.0 * (mean["on"] - mean["off"]) / mean["off"], max(diffs) - min(diffs), max(ms["off"]) - min(ms["off"])))
    lines.append("marked: %d convolutions, %.2f M weights (%.1f MB); shapes %s" %
                 (len(sn.convs), n_w / 1e6, n_w * 4 / 1e6, ", ".join("%dx%d" % (c.weight.shape[0], c.weight[0].numel()) for c in sn.convs)))
    # the two calls alone, back to back on an otherwise idle device
    for c in sn.convs:
        c.weight.grad = torch.zeros_like(c.weight)
    for name, call in (("update()", sn.update), ("project()", sn.project)):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(50):
            call()
        e1.record()
        torch.cuda.synchronize()
        lines.append("%s alone, 50 back to back: %.1f us each" % (name, e0.elapsed_time(e1) * 1000.0 / 50))
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    open(out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--leg":
        sys.path.insert(0, ROOT)
        measure(int(sys.argv[2]), sys.argv[3])
    else:
        B = sys.argv[1] if len(sys.argv) > 1 else "70"
        out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "spectral_cost.txt")
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", B, out], cwd=ROOT, timeout=LIMIT_S).returncode      # a fresh child under its own time limit
        if rc != 0:
            sys.exit("spectral_cost: the measuring leg ended with status %d; nothing else is started" % rc)
