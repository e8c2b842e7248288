"""What the device-side log costs: one process, isogd-depth at B = 70, fp32, the as-written schedule, three arms alternated in blocks on ONE
StepRunner — a run has one, and an arm is that runner with `monitor` / `sync_losses` set (tools/layer_table.py's protocol per block: --warm untimed iterations,
then --reps timed ones; the arms take turns --rounds times, so drift of the box hits all three):

  (a) plain     no monitor: the iteration as it is without this feature
  (b) monitor   trainer.build_monitor(interval=--interval) handed to StepRunner
  (c) sync      sync_losses=True: the reference's four loss.cpu().item() reads per iteration (trainer.py:326-328,363)

and the rate of dcv_hist_u8 on an all-background clip batch (every byte in one bin) next to a noise batch.  Prints ms per iteration per arm (median over the rounds
of the blocks' means) and one JSON line; --out writes the JSON to a file.

    python tools/monitor_overhead.py [--batch 70] [--rounds 4] [--out profiles/monitor_overhead.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument("--config", default="isogd-depth")
ap.add_argument("--batch", type=int, default=70)
ap.add_argument("--interval", type=int, default=100)
ap.add_argument("--warm", type=int, default=10)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--rounds", type=int, default=4)      # 4 x (10 + 20) iterations per arm: the monitor arm rolls once at interval 100
ap.add_argument("--hist-clips", type=int, default=64)
ap.add_argument("--no-arms", action="store_true", help="the histogram rates only")
ap.add_argument("--out", default="")
a = ap.parse_args()

from dcvgan_amd import monitor, native, trainer      # noqa: E402
from dcvgan_amd.configs import CONFIGS      # noqa: E402

native.lib()
native.set_precision("fp32")
dev = torch.device("cuda:0")
result = {"config": a.config, "batch": a.batch, "interval": a.interval, "warm": a.warm, "reps": a.reps, "rounds": a.rounds, "device": torch.cuda.get_device_name(0)}

if not a.no_arms:
    cfg = CONFIGS[a.config].scaled(batchsize=a.batch)
    torch.manual_seed(cfg.seed)
    models = trainer.build_models(cfg, dev)
    opts = trainer.build_optimizers(cfg, models)
    loss = trainer.build_loss(cfg)
    mon = trainer.build_monitor(cfg, models, opts, interval=a.interval)
    runner = trainer.StepRunner(cfg, models, opts, loss)
    arms = {"plain": dict(monitor=None, sync_losses=False), "monitor": dict(monitor=mon, sync_losses=False), "sync": dict(monitor=None, sync_losses=True)}
    g = torch.Generator().manual_seed(cfg.seed)
    lo, hi = (-0.5, 0.5) if cfg.channel == 2 else (-1.0, 1.0)
    xc = (torch.rand(a.batch, 3, cfg.video_length, 64, 64, generator=g) * 2 - 1).to(dev)
    xg = (torch.rand(a.batch, cfg.channel, cfg.video_length, 64, 64, generator=g) * (hi - lo) + lo).to(dev)
    blocks = {k: [] for k in arms}
    launches = {}
    records = 0
    for r in range(a.rounds):
        for name, arm in arms.items():
            runner.monitor, runner.sync_losses = arm["monitor"], arm["sync_losses"]
            for i in range(a.warm):
                runner.step(xc, xg, i % cfg.video_length)
            torch.cuda.synchronize()
            n0, t0 = native.launch_count(), time.perf_counter()
            for i in range(a.reps):
                runner.step(xc, xg, i % cfg.video_length)
            torch.cuda.synchronize()
            blocks[name].append((time.perf_counter() - t0) / a.reps * 1e3)
            launches[name] = (native.launch_count() - n0) / a.reps
            if name == "monitor":
                records += len(mon.poll())
    records += len(mon.drain())
    result["ms_per_iteration"] = {k: statistics.median(v) for k, v in blocks.items()}
    result["ms_per_iteration_blocks"] = blocks
    result["launches_per_iteration"] = launches
    result["monitor_minus_plain_ms"] = result["ms_per_iteration"]["monitor"] - result["ms_per_iteration"]["plain"]
    result["sync_minus_plain_ms"] = result["ms_per_iteration"]["sync"] - result["ms_per_iteration"]["plain"]
    result["records_published"] = records
    for k, v in result["ms_per_iteration"].items():
        print(f"{k:8s} {v:9.3f} ms / iteration   (blocks {', '.join(f'{b:.3f}' for b in blocks[k])}; {launches[k]:.2f} launches)")
    print(f"monitor - plain {result['monitor_minus_plain_ms']:+.3f} ms, sync - plain {result['sync_minus_plain_ms']:+.3f} ms, {records} records published")


def hist_rate(x):
    counts = torch.empty(256, dtype=torch.int64, device=dev)
    for _ in range(a.warm):
        monitor.hist_u8(x, 0, counts)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.reps):
        monitor.hist_u8(x, 0, counts)
    e1.record()
    e1.synchronize()
    ms = e0.elapsed_time(e1) / a.reps
    n = x.shape[0] * x.shape[2] * x.shape[3] * x.shape[4]
    assert int(counts.sum()) == n
    return {"ms": ms, "bytes_counted": n, "GB_per_s": n / ms * 1e-6}


shape = (a.hist_clips, 3, 16, 64, 64)
g = torch.Generator().manual_seed(1)
result["hist_u8"] = {"shape": list(shape), "background": hist_rate(torch.full(shape, 255, dtype=torch.uint8).to(dev)),
                     "noise": hist_rate(torch.randint(0, 256, shape, generator=g, dtype=torch.uint8).to(dev))}
for k in ("background", "noise"):
    h = result["hist_u8"][k]
    print(f"dcv_hist_u8 {k:10s} {h['ms'] * 1e3:8.1f} us for {h['bytes_counted']} bytes of channel 0 of {shape}: {h['GB_per_s']:.1f} GB/s (zeroing launch included)")
print(json.dumps(result))
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
