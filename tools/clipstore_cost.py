"""What the device-resident dataset costs: isogd-depth in fp32 at B = 70 (or argv[1]), a store of 1,500 videos of 16 .. 64 frames of 64 x 64 colour +
grey depth (about 1 GB: four times the Infinity Cache).
(a) The gather alone: dcv_clipstore_gather for both streams under a table, against dataprep.decode_color + decode_depth on the SAME bytes already contiguous on the
    device (the host-gathered batch of that table), alternating legs of back-to-back calls, device events; then the gather under a fresh table every call (its
    windows come from HBM, not from the cache), and the draw alone.
(b) The whole iteration: one StepRunner, 10 warm-up iterations, then alternating pairs of legs fed the same two tensors every iteration and fed by the sampler
    (draw + two gathers per iteration), device events around each leg.
The measuring leg is a fresh child process under its own time limit; a failure ends the script there.
Usage: python tools/clipstore_cost.py [B] [out.txt]      (default out: profiles/clipstore_cost.txt; the record also goes to stdout)"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARM, LEG, PAIRS = 10, 20, 3
CALLS = 1000         # back-to-back calls per leg of (a)
VIDEOS = 1500
LIMIT_S = 540


def measure(B, out):
    import datetime
    import time
    import numpy as np
    import torch
    from dcvgan_amd import clipstore, dataprep, native, trainer
    from dcvgan_amd.configs import CONFIGS
    native.lib()
    dev = torch.device("cuda:0")
    cfg = CONFIGS["isogd-depth"].scaled(batchsize=B)
    T, H, W = cfg.video_length, cfg.image_size, cfg.image_size
    counts = np.random.default_rng(0).integers(T, 65, size=VIDEOS).tolist()
    F = sum(counts)
    # random bytes made on the host in slabs (set-up, not timed); the packed tensors are adopted as they are
    color = torch.empty((F, H, W, 3), dtype=torch.uint8, device=dev)
    depth = torch.empty((F, H, W, 1), dtype=torch.uint8, device=dev)
    g = torch.Generator().manual_seed(1)
    for a in range(0, F, 8192):
        n = min(8192, F - a)
        color[a:a + n].copy_(torch.randint(0, 256, (n, H, W, 3), dtype=torch.uint8, generator=g))
        depth[a:a + n].copy_(torch.randint(0, 256, (n, H, W, 1), dtype=torch.uint8, generator=g))
    st = clipstore.ClipStore.from_packed(color, depth, counts, T, "depth")
    sampler = trainer.build_clip_sampler(cfg, st, seed=3, rank=0, world=1)
    lines = ["clip store cost: isogd-depth fp32, B = %d, %d videos, %d frames of %d x %d, store %.2f GB; one MI355X (%s), %s; library %s" %
             (B, VIDEOS, F, H, W, st.nbytes / 1e9, torch.cuda.get_device_name(0), datetime.date.today().isoformat(), native.csrc_digest()[:12])]

    host = [0.0]

    def timed(fn, n):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        h0 = time.perf_counter()
        for _ in range(n):
            fn()
        host[0] = (time.perf_counter() - h0) * 1e6 / n      # us the host takes to enqueue one call: a leg is a device time only where it is above this
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1000.0 / n      # us per call

    # ---- (a) the gather alone -------------------------------------------------------------------------------------------------------------------------------
    table = sampler.draw()
    rows = table.cpu().numpy().tolist()
    starts = st.starts_host
    idx = torch.tensor([starts[c] + t0 + t for c, t0 in rows for t in range(T)], dtype=torch.int64, device=dev)
    fc, fd = color[idx].reshape(B, T, H, W, 3).contiguous(), depth[idx].reshape(B, T, H, W, 1).contiguous()      # the same bytes, contiguous
    got = st.gather(table)
    same = torch.equal(got[0], dataprep.decode_color(fc)) and torch.equal(got[1], dataprep.decode_depth(fd))
    gather = lambda: st.gather(table)
    decode = lambda: (dataprep.decode_color(fc), dataprep.decode_depth(fd))
    for fn in (gather, decode):
        timed(fn, 20)
    nbytes = B * T * H * W * 4 * (1 + 4)      # 4 bytes per pixel read, 4 fp32 planes per pixel written
    lines.append("(a) gather of one batch (colour + depth, 2 launches) against decode_color + decode_depth (2 launches) on the same bytes, contiguous; outputs equal: %s; "
                 "%d calls per leg, %.1f MB read + written per batch" % (same, CALLS, nbytes / 1e6))
    us = {"gather": [], "decode": []}
    for p in range(PAIRS):
        a = timed(gather, CALLS); ha = host[0]
        b = timed(decode, CALLS); hb = host[0]
        us["gather"].append(a); us["decode"].append(b)
        lines.append("pair %d: gather %.1f us (%.2f TB/s; host enqueue %.1f us) | decode %.1f us (%.2f TB/s; host enqueue %.1f us) | ratio %.3f" %
                     (p + 1, a, nbytes / a / 1e6, ha, b, nbytes / b / 1e6, hb, a / b))
    mg, md = sum(us["gather"]) / PAIRS, sum(us["decode"]) / PAIRS
    lines.append("mean: gather %.1f us, decode %.1f us, ratio %.3f; spread of the gather legs %.1f us, of the decode legs %.1f us" %
                 (mg, md, mg / md, max(us["gather"]) - min(us["gather"]), max(us["decode"]) - min(us["decode"])))
    tables = []
    for i in range(CALLS):      # fresh windows every call: 1000 x 18 MB of frames out of a 1 GB store do not come from the cache
        sampler.epoch, sampler.iteration = i // len(sampler), i % len(sampler)
        tables.append(sampler.draw())
    sampler.epoch, sampler.iteration = 0, 0
    it = iter(tables)
    fresh = timed(lambda: st.gather(next(it)), CALLS)
    lines.append("gather under a fresh table every call (windows from HBM): %.1f us (%.2f TB/s)" % (fresh, nbytes / fresh / 1e6))
    lines.append("draw alone (1 launch, %d rows): %.1f us" % (B, timed(sampler.draw, CALLS)))

    # ---- (b) the whole iteration ----------------------------------------------------------------------------------------------------------------------------
    torch.manual_seed(1)
    models = trainer.build_models(cfg, dev)
    opts = trainer.build_optimizers(cfg, models)
    runner = trainer.StepRunner(cfg, models, opts, trainer.build_loss(cfg))
    xc, xg = got
    t_rand = np.random.default_rng(5).integers(0, T, size=4096).tolist()      # np.random.randint(0, video_length) of the reference's loop, drawn ahead
    k = [0]

    def leg(arm, n):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        c0 = native.launch_count()
        e0.record()
        for _ in range(n):
            if arm == "sampler":
                b = sampler.next_batch()
                runner.step(b["color"], b["depth"], t_rand[k[0] % 4096])
            else:
                runner.step(xc, xg, t_rand[k[0] % 4096])
            k[0] += 1
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n, (native.launch_count() - c0) / n

    leg("tensors", WARM)
    leg("sampler", 2)
    lines.append("(b) the whole iteration, one runner, %d warm-up iterations, %d alternating pairs of %d iterations, device events" % (WARM, PAIRS, LEG))
    ms, diffs = {"tensors": [], "sampler": []}, []
    for p in range(PAIRS):
        row = {}
        for arm in ("tensors", "sampler"):
            row[arm] = leg(arm, LEG)
            ms[arm].append(row[arm][0])
        diffs.append(row["sampler"][0] - row["tensors"][0])
        lines.append("pair %d: the same tensors %.2f ms / iteration (%.0f library launches) | sampler %.2f ms (%.0f launches) | difference %+.3f ms" %
                     (p + 1, row["tensors"][0], row["tensors"][1], row["sampler"][0], row["sampler"][1], diffs[-1]))
    mean = {a: sum(v) / len(v) for a, v in ms.items()}
    lines.append("mean: the same tensors %.2f ms, sampler %.2f ms, difference %+.3f ms (%+.2f %%); spread of the pairs' differences %.3f ms, of the tensor legs %.2f ms" %
                 (mean["tensors"], mean["sampler"], mean["sampler"] - mean["tensors"], 100.0 * (mean["sampler"] - mean["tensors"]) / mean["tensors"],
                  max(diffs) - min(diffs), max(ms["tensors"]) - min(ms["tensors"])))
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    open(out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--leg":
        sys.path.insert(0, ROOT)
        measure(int(sys.argv[2]), sys.argv[3])
    else:
        B = sys.argv[1] if len(sys.argv) > 1 else "70"
        out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "clipstore_cost.txt")
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", B, out], cwd=ROOT, timeout=LIMIT_S).returncode      # a fresh child under its own time limit
        if rc != 0:
            sys.exit("clipstore_cost: the measuring leg ended with status %d; nothing else is started" % rc)
