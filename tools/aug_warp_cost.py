"""What the augmentation's interpolated warps and saturation cost, by the method of tools/aug_cost.py: isogd-depth in fp32 at B = 70 (or argv[1]),
10 warm-up iterations per arm, then three alternating rounds of 20 iterations of (a) augmentation off, (b) the exact ops only, (c) all nine ops — three runners over
three copies of the models, the same data, adaptive mode from p = 0.5 — timed with device events around each leg; then the forward and the adjoint alone on one clip
pair, 20 back to back, for their achieved rate (bytes = one read and one write of the pair, whatever the taps re-read).  The measuring leg is a fresh child process
under its own time limit; a failure ends the script there.
Usage: python tools/aug_warp_cost.py [B] [out.txt]      (default out: profiles/aug_warp_cost.txt; the record also goes to stdout)"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARM, LEG, ROUNDS = 10, 20, 3
LIMIT_S = 540
ARMS = ("off", "exact", "all")
ALL_OPS = ("flip", "translate", "cutout", "colour", "scale", "rotate", "aniso", "subpixel", "saturation")


def measure(B, out):
    import copy
    import torch
    from dcvgan_amd import augment, native, trainer
    from dcvgan_amd.configs import CONFIGS
    native.lib()
    dev = torch.device("cuda:0")
    cfg = CONFIGS["isogd-depth"].scaled(batchsize=B)
    torch.manual_seed(1)
    models = {"off": trainer.build_models(cfg, dev)}
    models["exact"], models["all"] = copy.deepcopy(models["off"]), copy.deepcopy(models["off"])
    opts = {a: trainer.build_optimizers(cfg, models[a]) for a in ARMS}
    augs = {"off": None,
            "exact": trainer.build_augment(cfg, models["exact"], opts["exact"], p=0.5, adaptive=True, seed=3),
            "all": trainer.build_augment(cfg, models["all"], opts["all"], p=0.5, adaptive=True, seed=3, ops=ALL_OPS)}
    runners = {a: trainer.StepRunner(cfg, models[a], opts[a], trainer.build_loss(cfg), augment=augs[a]) for a in ARMS}
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

    for arm in ARMS:
        leg(arm, WARM)
    lines = ["warp augmentation cost: isogd-depth fp32, B = %d, %d warm-up iterations per arm, %d alternating rounds of %d iterations, device events; library %s" %
             (B, WARM, ROUNDS, LEG, native.csrc_digest()[:12])]
    ms = {a: [] for a in ARMS}
    for r in range(ROUNDS):
        row = {a: leg(a, LEG) for a in ARMS}
        for a in ARMS:
            ms[a].append(row[a][0])
        lines.append("round %d: off %.2f ms / iteration (%.0f library launches) | exact ops %.2f ms (%.0f) | all ops %.2f ms (%.0f) | exact - off %+.3f ms, all - off %+.3f ms, "
                     "all - exact %+.3f ms" % (r + 1, row["off"][0], row["off"][1], row["exact"][0], row["exact"][1], row["all"][0], row["all"][1],
                                               row["exact"][0] - row["off"][0], row["all"][0] - row["off"][0], row["all"][0] - row["exact"][0]))
    mean = {a: sum(v) / len(v) for a, v in ms.items()}
    d_all = [a - o for a, o in zip(ms["all"], ms["off"])]
    d_ex = [a - o for a, o in zip(ms["exact"], ms["off"])]
    lines.append("mean: off %.2f ms, exact ops %.2f ms (%+.3f ms), all ops %.2f ms (%+.3f ms, %+.2f %%); spread of the rounds' differences: exact %.3f ms, all %.3f ms; "
                 "of the off legs %.2f ms" % (mean["off"], mean["exact"], mean["exact"] - mean["off"], mean["all"], mean["all"] - mean["off"],
                                              100.0 * (mean["all"] - mean["off"]) / mean["off"], max(d_ex) - min(d_ex), max(d_all) - min(d_all),
                                              max(ms["off"]) - min(ms["off"])))
    lines.append("state after the run: exact p = %.4f, all p = %.4f, draws %d / %d" % (augs["exact"].p(), augs["all"].p(), augs["exact"].draws, augs["all"].draws))

    # the kernels alone: one pair (geometry + colour) in the generators' (B, T, C, H, W) layout, 20 back to back on an otherwise idle device
    pair_bytes = 2 * 4 * (xg.numel() + xc.numel())
    a, b = (t.permute(0, 2, 1, 3, 4).contiguous().permute(0, 2, 1, 3, 4) for t in (xg, xc))
    fixed = {p: trainer.build_augment(cfg, models["all"], opts["all"], p=p, adaptive=False, seed=5, ops=ALL_OPS) for p in (0.0, 0.5, 1.0)}
    cases = [("exact entries, p = 0.5 table", augs["exact"].draw(B, 64, 64))] + [("warp entries, p = %.1f table" % p, fixed[p].draw(B, 64, 64)) for p in (0.0, 0.5, 1.0)]

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1000.0 / 20

    for label, table in cases:
        wide = table.shape[1] == augment.WARP_ROW_WORDS
        warp_rows = int((table[:, 8] != 0).sum()) if wide else 0
        fwd = (lambda: (augment.warp_apply(a, table, False), augment.warp_apply(b, table, True))) if wide else (lambda: (augment.apply(a, table, False), augment.apply(b, table, True)))
        bwd = (lambda: (augment.warp_apply_backward(a, table, False), augment.warp_apply_backward(b, table, True))) if wide else \
              (lambda: (augment.apply_backward(a, table, False), augment.apply_backward(b, table, True)))
        for what, fn in (("forward", fwd), ("adjoint", bwd)):
            us = timed(fn)
            lines.append("%s alone, %s (%d of %d rows interpolate), 20 back to back: %.1f us per pair, %.1f MB moved -> %.2f TB/s" %
                         (what, label, warp_rows, B, us, pair_bytes / 1e6, pair_bytes / us / 1e6))
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    open(out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--leg":
        sys.path.insert(0, ROOT)
        measure(int(sys.argv[2]), sys.argv[3])
    else:
        B = sys.argv[1] if len(sys.argv) > 1 else "70"
        out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "aug_warp_cost.txt")
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", B, out], cwd=ROOT, timeout=LIMIT_S).returncode      # a fresh child under its own time limit
        if rc != 0:
            sys.exit("aug_warp_cost: the measuring leg ended with status %d; nothing else is started" % rc)
