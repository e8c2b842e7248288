"""What the clip augmentation costs: isogd-depth in fp32 at B = 70 (or argv[1]), 10 warm-up iterations per arm, then three alternating pairs of 20 iterations with
the augmentation off and on (two runners over two copies of the models, the same data; adaptive mode from p = 0.5), timed with device events around each leg; then the
gather alone on one clip pair, back to back, for its HBM rate.  The measuring leg is a fresh child process under its own time limit; a failure ends the script there.
Usage: python tools/aug_cost.py [B] [out.txt]      (default out: profiles/aug_cost.txt; the record also goes to stdout)"""
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
    aug = trainer.build_augment(cfg, models["on"], opts["on"], p=0.5, adaptive=True, seed=3)
    runners = {"off": trainer.StepRunner(cfg, models["off"], opts["off"], trainer.build_loss(cfg)),
               "on": trainer.StepRunner(cfg, models["on"], opts["on"], trainer.build_loss(cfg), augment=aug)}
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
    lines = ["augmentation cost: isogd-depth fp32, B = %d, %d warm-up iterations per arm, %d alternating pairs of %d iterations, device events; library %s" %
             (B, WARM, PAIRS, LEG, native.csrc_digest()[:12])]
    ms, diffs = {"off": [], "on": []}, []
    for p in range(PAIRS):
        row = {}
        for arm in ("off", "on"):
            row[arm] = leg(arm, LEG)
            ms[arm].append(row[arm][0])
        diffs.append(row["on"][0] - row["off"][0])
        lines.append("pair %d: augmentation off %.2f ms / iteration (%.0f library launches) | on %.2f ms (%.0f launches) | difference %+.3f ms" %
                     (p + 1, row["off"][0], row["off"][1], row["on"][0], row["on"][1], diffs[-1]))
    mean = {a: sum(v) / len(v) for a, v in ms.items()}
    lines.append("mean: off %.2f ms, on %.2f ms, augmentation %+.3f ms (%+.2f %%); spread of the pairs' differences %.3f ms, of the off legs %.2f ms" %
                 (mean["off"], mean["on"], mean["on"] - mean["off"], 100.0 * (mean["on"] - mean["off"]) / mean["off"], max(diffs) - min(diffs), max(ms["off"]) - min(ms["off"])))
    lines.append("state after the run: p = %.4f, adjustments %d, draws %d" % (aug.p(), aug.adjusts(), aug.draws))
    # the gather alone: one pair (geometry + colour), forward, back to back on an otherwise idle device; bytes = one read and one write of the pair
    pair_bytes = 2 * 4 * (xg.numel() + xc.numel())
    table = aug.draw(B, 64, 64)
    for label, a, b in (("contiguous pair", xg, xc),
                        ("generators' (B, T, C, H, W) layout", xg.permute(0, 2, 1, 3, 4).contiguous().permute(0, 2, 1, 3, 4), xc.permute(0, 2, 1, 3, 4).contiguous().permute(0, 2, 1, 3, 4))):
        aug(a, b, table=table)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            aug(a, b, table=table)
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1000.0 / 20
        lines.append("apply alone, %s, 20 back to back: %.1f us per pair, %.1f MB moved -> %.2f TB/s" % (label, us, pair_bytes / 1e6, pair_bytes / us / 1e6))
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    open(out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--leg":
        sys.path.insert(0, ROOT)
        measure(int(sys.argv[2]), sys.argv[3])
    else:
        B = sys.argv[1] if len(sys.argv) > 1 else "70"
        out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "aug_cost.txt")
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", B, out], cwd=ROOT, timeout=LIMIT_S).returncode      # a fresh child under its own time limit
        if rc != 0:
            sys.exit("aug_cost: the measuring leg ended with status %d; nothing else is started" % rc)
