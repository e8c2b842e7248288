"""What a RunState capture costs: isogd-depth in fp32 at B = 70 (or argv[1]) with the generators' EMA twins, one process, 10 warm-up iterations, then three
alternating pairs of 20 iterations without and with a capture() after every iteration (the same runner, the same data), timed with device events around each
leg; then capture() alone, fingerprint() alone and one save() to a file.
Usage: python tools/runstate_cost.py [B] [out.txt]      (the record also goes to stdout; default out: profiles/runstate_cost.txt)"""
import os
import sys
import tempfile
import time
sys.path.insert(0, '.')
import torch
from dcvgan_amd import native, trainer
from dcvgan_amd.configs import CONFIGS

B = int(sys.argv[1]) if len(sys.argv) > 1 else 70
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join("profiles", "runstate_cost.txt")
WARM, LEG, PAIRS = 10, 20, 3
native.lib()
dev = torch.device("cuda:0")
cfg = CONFIGS["isogd-depth"].scaled(batchsize=B)
torch.manual_seed(1)
models = trainer.build_models(cfg, dev)
opts = trainer.build_optimizers(cfg, models)
ema = trainer.build_ema(cfg, models, opts)
runner = trainer.StepRunner(cfg, models, opts, trainer.build_loss(cfg), ema=ema)
rs = trainer.build_run_state(cfg, models, opts, runner=runner, ema=ema)
g = torch.Generator().manual_seed(2)
xc = (torch.rand(B, 3, 16, 64, 64, generator=g) * 2 - 1).to(dev); xg = (torch.rand(B, cfg.channel, 16, 64, 64, generator=g) * 2 - 1).to(dev)


def leg(capture, n):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    c0 = native.launch_count()
    e0.record()
    for i in range(n):
        runner.step(xc, xg, i % 16)
        if capture:
            rs.capture()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n, (native.launch_count() - c0) / n


def alone(call, n=20):
    call()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(n):
        call()
    host = (time.perf_counter() - t0) / n
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n, host * 1e3


leg(True, WARM)
nbytes, entries, per = rs.arena_bytes(), len(rs.manifest()), rs.launches_per_capture()
lines = ["runstate cost: isogd-depth fp32 with EMA twins, B = %d, %d warm-up iterations, %d alternating pairs of %d iterations, device events; library %s" %
         (B, WARM, PAIRS, LEG, native.csrc_digest()[:12]),
         "snapshot: %d entries, %.1f MB, %d launches per capture" % (entries, nbytes / 1e6, per)]
ms = {False: [], True: []}
for p in range(PAIRS):
    row = {}
    for arm in (False, True):
        t, launches = leg(arm, LEG)
        ms[arm].append(t); row[arm] = (t, launches)
    lines.append("pair %d: no capture %.2f ms / iteration (%.0f library launches) | a capture per iteration %.2f ms (%.0f launches) | difference %+.2f ms" %
                 (p + 1, row[False][0], row[False][1], row[True][0], row[True][1], row[True][0] - row[False][0]))
mean = {a: sum(v) / len(v) for a, v in ms.items()}
lines.append("mean: without %.2f ms, with %.2f ms, capture %+.2f ms (%+.2f %%); spread of the legs without %.2f ms" %
             (mean[False], mean[True], mean[True] - mean[False], 100.0 * (mean[True] - mean[False]) / mean[False], max(ms[False]) - min(ms[False])))
dev_ms, host_ms = alone(rs.capture)
lines.append("capture() alone, back to back: %.3f ms on the device (%.2f TB/s read + written), %.3f ms of host time per call" % (dev_ms, 2 * nbytes / dev_ms / 1e9, host_ms))
dev_ms, host_ms = alone(rs.fingerprint)
lines.append("fingerprint() alone, back to back: %.3f ms on the device (%.2f TB/s read), %.3f ms of host time per call" % (dev_ms, nbytes / dev_ms / 1e9, host_ms))
snap = rs.capture()
torch.cuda.synchronize()
with tempfile.TemporaryDirectory() as d:
    path = os.path.join(d, "run.pt")
    t0 = time.perf_counter()
    snap.save(path)
    dt = time.perf_counter() - t0
    lines.append("one save(): %.2f s for a file of %.1f MB (device -> pinned host copy, then torch.save)" % (dt, os.path.getsize(path) / 1e6))
print("\n".join(lines))
if OUT:
    open(OUT, "w").write("\n".join(lines) + "\n")
