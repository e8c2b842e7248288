"""What on-device evaluation costs, on one MI355X, with the protocol of tools/layer_table.py: HIP events around REPS timed calls after WARM untimed ones.
(a) dcv_eval_moments_update at (n, D) = (100, 2048) — one batch of an evaluation — and at (10000, 2048), where the fp64 matrix pipe's rate shows.
(b) dcv_eval_kid_sums at the defaults: 100 subsets of 1000, D = 2048 (and the draw alone).
(c) dcv_eval_inception_update at (100, 400).
(d) One Evaluator.evaluate of 1000 samples of isogd-depth in batches of 50 with all three metrics, against the same sampling loop alone; the extractor is a stand-in
    that returns free views of the clip (2048 features, 400 logits), so the difference is this module's launches and its host finalisation.
(e) The k-nearest-neighbour metrics at 10000 x 10000, D = 2048: dcv_eval_knn_radii and dcv_eval_manifold_counts with k = 3 and 5 (2 n^2 D FLOP each,
    all of it executed: no symmetry is used), the norms, and manifold_metrics end to end; dcv_eval_kid_sums of (b), timed in the same process, is the yardstick.
(f) PRD's k-means at the workload's size, 10000 + 10000 rows, D = 2048, 20 clusters x 10 runs, 20 iterations: one dcv_eval_prd_assign, one
    dcv_eval_prd_update (and across row_splits), prd_metrics end to end; beside them in the same process a plain read of the two feature matrices (torch's sum, as
    tools/hbm_probe.py reads, and dcv_eval_row_norms), dcv_eval_moments_update at (20000, 2048) — the update's contraction — and dcv_eval_knn_radii — the
    assignment's sweep.  `--legs f` runs this leg alone and appends its record to the file.
FLOP counts are the nominal ones of the full matrices (2 n D^2 for the Gram, 3 * subsets * 2 m^2 D for the kernel distance); the kernels execute the upper tiles of
the symmetric blocks only.  The measuring leg is a fresh child process under its own time limit; a failure ends the script there.
Usage: python tools/eval_cost.py [--legs abcdef] [out.txt]      (default out: profiles/eval_cost.txt; the record also goes to stdout)"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARM, REPS = 10, 20
LIMIT_S = 540


def measure(out, legs="abcdef"):
    import datetime
    import time
    import torch
    from dcvgan_amd import evaluation as E, native, trainer
    from dcvgan_amd.configs import CONFIGS
    native.lib()
    dev = torch.device("cuda:0")
    lines = ["evaluation cost: one MI355X (%s), %s; HIP events, %d timed calls after %d untimed; library %s" %
             (torch.cuda.get_device_name(0), datetime.date.today().isoformat(), REPS, WARM, native.csrc_digest()[:12])]

    def timed(fn, reps=REPS, warm=WARM):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps      # ms per call

    g = torch.Generator().manual_seed(1)
    D = 2048
    if legs == "f":
        prd_leg(lines, timed, g, dev, D)
        print("\n".join(lines))
        open(out, "a").write("\n" + "\n".join(lines) + "\n")
        return
    # ---- (a) the moments ----
    for n, reps, warm in ((100, REPS, WARM), (10000, 5, 2)):
        x = torch.randn(n, D, generator=g).to(dev)
        fm = E.FeatureMoments(D, dev)
        ms = timed(lambda: fm.update(x), reps, warm)
        gflop = 2.0 * n * D * D / 1e9
        lines.append("(a) dcv_eval_moments_update (%d, %d): %.3f ms per call, %.2f GFLOP nominal -> %.2f TFLOP/s fp64 (%d timed after %d)" %
                     (n, D, ms, gflop, gflop / ms, reps, warm))
    # ---- (b) the kernel distance ----
    fa, fb = torch.randn(10000, D, generator=g).to(dev), (torch.randn(10000, D, generator=g) + 0.1).to(dev)
    table = E.kid_draw(10000, 10000, 100, 1000, 0, dev)
    ms = timed(lambda: E.kid_sums(fa, fb, table), 5, 2)
    tflop = 3 * 100 * 2.0 * 1000 * 1000 * D / 1e12
    lines.append("(b) dcv_eval_kid_sums, 100 subsets of 1000, D = %d, rows gathered from 2 x 10000: %.2f ms per call, %.2f TFLOP nominal -> %.2f TFLOP/s fp64 "
                 "(5 timed after 2)" % (D, ms, tflop, tflop / ms * 1e3))
    lines.append("    dcv_eval_kid_draw alone (100 x 2 x 1000 rows): %.1f us" % (timed(lambda: E.kid_draw(10000, 10000, 100, 1000, 0, dev)) * 1e3))
    h0 = time.perf_counter()
    kid = E.kernel_distance(fa, fb)
    lines.append("    kernel_distance end to end (draw, sums, host read): %.1f ms; KID %.3e +- %.1e" % ((time.perf_counter() - h0) * 1e3, kid[0], kid[1]))
    # ---- (c) the Inception sums ----
    z = (torch.randn(100, 400, generator=g) * 3).to(dev)
    st = E.InceptionStats(400, dev)
    lines.append("(c) dcv_eval_inception_update (100, 400), 2 launches: %.1f us per call" % (timed(lambda: st.update(z)) * 1e3))
    # ---- (d) one evaluation ----
    cfg = CONFIGS["isogd-depth"]
    torch.manual_seed(1)
    models = trainer.build_models(cfg, dev)

    def extractor(xc):
        flat = xc.permute(0, 2, 1, 3, 4).reshape(xc.shape[0], -1)
        return flat[:, :D], flat[:, D:D + 400]

    ev = trainer.build_evaluator(cfg, models, extractor)
    T, S = cfg.video_length, cfg.image_size
    for _ in range(20):
        ev.observe_real((torch.rand(50, 3, T, S, S, generator=g) * 2 - 1).to(dev))

    def sample_only():
        with torch.no_grad():
            for _ in range(20):
                extractor(models["cgen"].forward_videos(models["ggen"].sample_videos(50)))
        torch.cuda.synchronize()

    ev.evaluate(num_samples=100, batchsize=50)      # warm-up
    sample_only()
    rows = []
    for _ in range(2):
        h0 = time.perf_counter(); l0 = E.launches()
        res = ev.evaluate(num_samples=1000, batchsize=50)
        t_eval = time.perf_counter() - h0
        n_launch = E.launches() - l0
        h0 = time.perf_counter()
        sample_only()
        rows.append((t_eval, time.perf_counter() - h0))
    h0 = time.perf_counter()
    E.frechet_distance(ev.real, ev.fake)
    t_fid = time.perf_counter() - h0
    lines.append("(d) Evaluator.evaluate, 1000 samples of isogd-depth in batches of 50, is + fid + kid (D = %d, K = 400, 1000 real clips observed before): "
                 "%.2f s / %.2f s wall clock in two runs, the same sampling loop alone %.2f s / %.2f s; %d launches of this module; of the rest the host's "
                 "frechet_distance (two symmetric eigenproblems of %d x %d) takes %.2f s" % (D, rows[0][0], rows[1][0], rows[0][1], rows[1][1], n_launch, D, D, t_fid))
    lines.append("    result: " + ", ".join("%s %.6g" % kv for kv in sorted(res.items())))
    # ---- (e) precision / recall and density / coverage ----
    n = 10000
    exe = tflop * 2.0 / 3.0 / ms * 1e3      # (b)'s executed rate: the upper tiles of the two symmetric blocks and the whole cross block, 2/3 of nominal
    lines.append("(e) k-nearest-neighbour metrics, %d x %d, D = %d (5 timed after 2; yardstick dcv_eval_kid_sums above: %.1f TFLOP/s executed)" % (n, n, D, exe))
    norm_a, norm_b = E.row_norms(fa), E.row_norms(fb)
    lines.append("    dcv_eval_row_norms (%d, %d): %.1f us" % (n, D, timed(lambda: E.row_norms(fa)) * 1e3))
    tf = 2.0 * n * n * D / 1e12
    for k in (3, 5):
        ms_k = timed(lambda: E.knn_radii(fa, k, norms=norm_a), 5, 2)
        rad = E.knn_radii(fa, k, norms=norm_a)
        ms_c = timed(lambda: E.manifold_counts(fb, fa, rad, norms_q=norm_b, norms_s=norm_a), 5, 2)
        lines.append("    k = %d: dcv_eval_knn_radii %.2f ms, %.2f TFLOP -> %.1f TFLOP/s fp64; dcv_eval_manifold_counts %.2f ms -> %.1f TFLOP/s fp64" %
                     (k, ms_k, tf, tf / ms_k * 1e3, ms_c, tf / ms_c * 1e3))
    for cs in (1, 2, 3, 4, 6):
        lines.append("    k = 5, col_splits %d: dcv_eval_knn_radii %.2f ms, dcv_eval_manifold_counts %.2f ms" %
                     (cs, timed(lambda: E.knn_radii(fa, 5, cs, norms=norm_a), 3, 1), timed(lambda: E.manifold_counts(fb, fa, rad, cs, norms_q=norm_b, norms_s=norm_a), 3, 1)))
    E.manifold_metrics(fa, fb)
    torch.cuda.synchronize()
    h0 = time.perf_counter(); l0 = E.launches()
    res = E.manifold_metrics(fa, fb)
    lines.append("    manifold_metrics end to end (k 3 and 5: norms, 3 radius vectors, 3 counts, reductions, host read): %.1f ms, %d launches; %s" %
                 ((time.perf_counter() - h0) * 1e3, E.launches() - l0, ", ".join("%s %.4f" % kv for kv in sorted(res.items()))))
    prd_leg(lines, timed, g, dev, D)
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    open(out, "w").write("\n".join(lines) + "\n")


def prd_leg(lines, timed, g, dev, D):
    """(f): 10000 + 10000 rows, 20 clusters x 10 runs, 20 iterations."""
    import time
    import torch
    from dcvgan_amd import evaluation as E, native
    n, C, R, T = 10000, 20, 10, 20
    fa, fb = torch.randn(n, D, generator=g).to(dev), (0.8 * torch.randn(n, D, generator=g) + 0.3).to(dev)
    both = torch.cat([fa, fb])
    mb = 2 * n * D * 4 / 1e6
    lines.append("(f) PRD's k-means, %d + %d rows, D = %d, %d clusters x %d runs (5 timed after 2 unless said otherwise)" % (n, n, D, C, R))
    ms = timed(lambda: (fa.sum(), fb.sum()))
    lines.append("    plain read of the two feature matrices (%.0f MB, torch sum x 2; they fit the 256 MB last-level cache): %.1f us -> %.2f TB/s" % (mb, ms * 1e3, mb / ms / 1e3))
    ms = timed(lambda: (E.row_norms(fa), E.row_norms(fb)))
    lines.append("    dcv_eval_row_norms of both sides: %.1f us -> %.2f TB/s" % (ms * 1e3, mb / ms / 1e3))
    fm = E.FeatureMoments(D, dev)
    ms = timed(lambda: fm.update(both), 5, 2)
    gf = 2.0 * 2 * n * D * D / 1e9
    lines.append("    dcv_eval_moments_update (%d, %d), the update's contraction: %.2f ms, %.1f GFLOP nominal -> %.1f TFLOP/s fp64" % (2 * n, D, ms, gf, gf / ms))
    norm_a, norm_b = E.row_norms(fa), E.row_norms(fb)
    ms = timed(lambda: E.knn_radii(fa, 3, norms=norm_a), 5, 2)
    tf = 2.0 * n * n * D / 1e12
    lines.append("    dcv_eval_knn_radii (%d rows, k = 3), the assignment's sweep: %.2f ms, %.2f TFLOP -> %.1f TFLOP/s fp64" % (n, ms, tf, tf / ms * 1e3))
    cent = E.prd_seed(fa, fb, C, R, 0)
    lines.append("    dcv_eval_prd_seed: %.1f us" % (timed(lambda: E.prd_seed(fa, fb, C, R, 0)) * 1e3))
    ms = timed(lambda: E.prd_assign(fa, fb, cent, norm_a, norm_b), 5, 2)
    nominal, issued = 2.0 * 2 * n * R * C * D / 1e9, 2.0 * 2 * n * (R // 2) * 64 * D / 1e9      # C = 20: two runs of 32 columns per 64-column tile
    lines.append("    dcv_eval_prd_assign (2 launches): %.3f ms; %.1f GFLOP nominal -> %.1f TFLOP/s fp64, %.1f GFLOP issued -> %.1f TFLOP/s" %
                 (ms, nominal, nominal / ms, issued, issued / ms))
    assign = E.prd_assign(fa, fb, cent, norm_a, norm_b)
    S0 = int(native.lib().dcv_eval_prd_update_workspace_bytes(2 * n, D, C, R, 0)) // (R * C * D * 8)
    for S in (0, 1, 2, 4, 8, 16, 32):
        ms = timed(lambda: E.prd_update(fa, fb, assign, cent.clone(), S, norm_a, norm_b), 5, 2)
        ms_clone = timed(lambda: cent.clone(), 5, 2)
        lines.append("    dcv_eval_prd_update (3 launches), row_splits %d%s: %.3f ms (a copy of the centroids, %.3f ms, taken off); %.1f GFLOP nominal -> %.1f TFLOP/s fp64" %
                     (S, " (the library's choice: S = %d)" % S0 if S == 0 else "", ms - ms_clone, ms_clone, nominal, nominal / (ms - ms_clone)))
    E.prd_metrics(fa, fb, C, R, T)
    torch.cuda.synchronize()
    rows = []
    for _ in range(3):
        h0 = time.perf_counter(); l0 = E.launches()
        res = E.prd_metrics(fa, fb, C, R, T)
        rows.append((time.perf_counter() - h0) * 1e3)
    lines.append("    prd_metrics end to end, %d iterations (norms, seed, %d x (assign, update), assign, count, one host read, the curve on the host): %s ms wall clock in "
                 "three runs, %d launches; %s" % (T, T, " / ".join("%.1f" % r for r in rows), E.launches() - l0, ", ".join("%s %.6f" % kv for kv in sorted(res.items()))))
    hist = E.prd_kmeans(fa, fb, C, R, 0)[0].cpu().numpy()
    h0 = time.perf_counter()
    E._prd_scores(hist)
    lines.append("    of that the host's curve and F_beta: %.2f ms" % ((time.perf_counter() - h0) * 1e3))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--leg":
        sys.path.insert(0, ROOT)
        measure(sys.argv[2], sys.argv[3])
    else:
        args = sys.argv[1:]
        legs = "abcdef"
        if args and args[0] == "--legs":
            legs, args = args[1], args[2:]
        if legs not in ("abcdef", "f"):
            sys.exit("eval_cost: --legs abcdef (all, the default) or f (the PRD leg alone, appended to the record)")
        out = args[0] if args else os.path.join(ROOT, "profiles", "eval_cost.txt")
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", out, legs], cwd=ROOT, timeout=LIMIT_S).returncode      # a fresh child under its own time limit
        if rc != 0:
            sys.exit("eval_cost: the measuring leg ended with status %d; nothing else is started" % rc)
