"""What the LeCam regulariser costs: isogd-depth in fp32 at B = 70 (or argv[1]), 10 warm-up iterations per arm, then three alternating pairs of 20 iterations with
lecam=None and with the regulariser on and active (two runners over two copies of the models, the same data), timed with device events around each leg; then the two
launches alone on logits of the iteration's sizes, back to back.  (tools/ab.sh alternates bench.py runs, and bench.py has no switch for an optional feature: the
pairs alternate inside one process instead, as tools/aug_cost.py's do.)  The measuring leg is a fresh child process under its own time limit; a failure ends the
script there.
Usage: python tools/lecam_cost.py [B] [out.txt]      (default out: profiles/lecam_cost.txt; the record also goes to stdout)"""
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
    lc = trainer.build_lecam(cfg, models["on"], opts["on"], weight=0.3, start=0)
    runners = {"off": trainer.StepRunner(cfg, models["off"], opts["off"], trainer.build_loss(cfg)),
               "on": trainer.StepRunner(cfg, models["on"], opts["on"], trainer.build_loss(cfg), lecam=lc)}
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
    lines = ["LeCam cost: isogd-depth fp32, B = %d, %d warm-up iterations per arm, %d alternating pairs of %d iterations, device events; library %s" %
             (B, WARM, PAIRS, LEG, native.csrc_digest()[:12])]
    ms, diffs = {"off": [], "on": []}, []
    for p in range(PAIRS):
        row = {}
        for arm in ("off", "on"):
            row[arm] = leg(arm, LEG)
            ms[arm].append(row[arm][0])
        diffs.append(row["on"][0] - row["off"][0])
        lines.append("pair %d: lecam=None %.2f ms / iteration (%.0f library launches) | on %.2f ms (%.0f launches) | difference %+.3f ms" %
                     (p + 1, row["off"][0], row["off"][1], row["on"][0], row["on"][1], diffs[-1]))
    mean = {a: sum(v) / len(v) for a, v in ms.items()}
    lines.append("mean: lecam=None %.2f ms, on %.2f ms, regulariser %+.3f ms (%+.2f %%); spread of the pairs' differences %.3f ms, of the lecam=None legs %.2f ms" %
                 (mean["off"], mean["on"], mean["on"] - mean["off"], 100.0 * (mean["on"] - mean["off"]) / mean["off"], max(diffs) - min(diffs), max(ms["off"]) - min(ms["off"])))
    words = lc.state_words()
    lines.append("state after the run: updates %s, active %s, anchors %s, last terms %s" %
                 ([w[2] for w in words], [w[3] for w in words], [tuple(round(v, 4) for v in a) for a in lc.anchor_values()], [round(float(v), 6) for v in lc.reg.cpu().tolist()]))
    # the two launches alone, on logits of the iteration's sizes (B; B x 4 x 4 x 4 for the 3-D discriminators is the upper end), back to back on an otherwise idle device
    sizes = [B, B * 64, B * 64]
    ys = [[torch.randn(n, device=dev) for n in sizes] for _ in range(2)]
    losses, dys = [torch.zeros((), device=dev) for _ in sizes], [[torch.zeros(n, device=dev) for n in sizes] for _ in range(2)]
    solo = trainer.build_lecam(cfg, models["on"], opts["on"], weight=0.3, start=0)
    for _ in range(3):
        solo._fold(ys[0], ys[1], losses, dys[0], dys[1])
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(20):
        solo._fold(ys[0], ys[1], losses, dys[0], dys[1])
    e1.record()
    torch.cuda.synchronize()
    nbytes = 4 * (4 * sum(sizes) + 2 * 2 * sum(sizes))      # sums reads 2 x, apply reads 2 x and reads + writes 2 gradients
    lines.append("the two launches alone, logits %s per side, 20 back to back: %.1f us per pair of launches, %.1f KB touched" %
                 (sizes, e0.elapsed_time(e1) * 1000.0 / 20, nbytes / 1e3))
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    open(out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--leg":
        sys.path.insert(0, ROOT)
        measure(int(sys.argv[2]), sys.argv[3])
    else:
        B = sys.argv[1] if len(sys.argv) > 1 else "70"
        out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "lecam_cost.txt")
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", B, out], cwd=ROOT, timeout=LIMIT_S).returncode      # a fresh child under its own time limit
        if rc != 0:
            sys.exit("lecam_cost: the measuring leg ended with status %d; nothing else is started" % rc)
