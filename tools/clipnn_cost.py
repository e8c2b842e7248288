"""What the nearest-training-clip search costs: clipnn.nearest_windows on a synthetic colour store of 120,000 frames of 64 x 64 x 3 (1.5 GB: six times
the Infinity Cache), n = 16 and n = 64 fp32 queries, k = 3; 20 timed calls after 5 untimed, device events.  Two floors are printed beside every row:
  - the store's bytes against the plain read rate of the SAME buffer (torch's sum over it, the method of tools/hbm_probe.py): the GEMM reads the store once per
    tile of 256 query frames, so a call moves ceil(n T / 256) x the store;
  - the int8 multiply-adds, n T x frames x H W C, against twice the dense bf16 MFMA peak (v_mfma_i32_32x32x32_i8 does the bf16 form's cycles at twice the K).
There is no pass mark: nothing earlier computes this.  The measuring leg is a fresh child process under its own time limit; a failure ends the script there.
Usage: python tools/clipnn_cost.py [out.txt]      (default out: profiles/clipnn_cost.txt; the record also goes to stdout)"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VIDEOS, FRAMES_PER_VIDEO, H, W, T, K_BEST = 1500, 80, 64, 64, 16, 3
WARM, CALLS = 5, 20
BF16_PEAK_MACS = 1.25e15      # 2.5 PFLOP/s dense
LIMIT_S = 420


def measure(out):
    import datetime
    import torch
    from dcvgan_amd import clipnn, clipstore, native
    native.lib()
    dev = torch.device("cuda:0")
    counts = [FRAMES_PER_VIDEO] * VIDEOS
    F = sum(counts)
    color = torch.empty((F, H, W, 3), dtype=torch.uint8, device=dev)
    depth = torch.zeros((F, H, W, 1), dtype=torch.uint8, device=dev)
    g = torch.Generator(device=dev).manual_seed(1)
    for a in range(0, F, 8192):      # random bytes (set-up, not timed)
        n = min(8192, F - a)
        color[a:a + n] = torch.randint(0, 256, (n, H, W, 3), dtype=torch.uint8, device=dev, generator=g)
    st = clipstore.ClipStore.from_packed(color, depth, counts, T, "depth")
    store_bytes = color.numel()

    def timed(fn):
        for _ in range(WARM):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(CALLS):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / CALLS      # ms per call

    as_f32 = color.view(-1).view(torch.float32)
    read_ms = timed(lambda: as_f32.sum())
    read_rate = store_bytes / read_ms / 1e9      # TB/s
    lines = ["clipnn cost: colour store of %d frames of %d x %d x 3 (%.2f GB), T = %d, k = %d, fp32 queries; %d timed calls after %d untimed, device events; one MI355X (%s), %s"
             % (F, H, W, store_bytes / 1e9, T, K_BEST, CALLS, WARM, torch.cuda.get_device_name(0), datetime.date.today().isoformat()),
             "plain read of the store (torch sum over the same buffer): %.3f ms, %.2f TB/s" % (read_ms, read_rate)]
    for n in (16, 64):
        q = (torch.randn((n * T, 3, H, W), device=dev, generator=g) * 0.5).view(n, T, 3, H, W).permute(0, 2, 1, 3, 4)
        launches = clipnn.launches_for(st, n, K_BEST)
        ms = timed(lambda: clipnn.nearest_windows(st, q, k=K_BEST))
        tiles = (n * T + 255) // 256
        rate = tiles * store_bytes / ms / 1e9
        macs = n * T * F * H * W * 3 / (ms * 1e-3)
        lines.append("n = %2d: %.3f ms per call (%d launches) | store bytes %.2f TB/s = %.0f %% of the plain read rate (%d pass%s over the store) | int8 MACs %.1f T/s = %.1f %% of "
                     "twice the bf16 peak | floors: read %.3f ms, MFMA %.3f ms" %
                     (n, ms, launches, rate, 100.0 * rate / read_rate, tiles, "" if tiles == 1 else "es", macs / 1e12, 100.0 * macs / (2 * BF16_PEAK_MACS),
                      tiles * read_ms, n * T * F * H * W * 3 / (2 * BF16_PEAK_MACS) * 1e3))
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    open(out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--leg":
        sys.path.insert(0, ROOT)
        measure(sys.argv[2])
    else:
        out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "clipnn_cost.txt")
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", out], cwd=ROOT, timeout=LIMIT_S).returncode      # a fresh child under its own time limit
        if rc != 0:
            sys.exit("clipnn_cost: the measuring leg ended with status %d; nothing else is started" % rc)
