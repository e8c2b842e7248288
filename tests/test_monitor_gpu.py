"""GPU: dcv_monitor_observe / dcv_monitor_roll / dcv_hist_u8 / dcv_video_grid_u8 against their numpy mirrors (dcvgan_amd.monitor, checked on the CPU by
tests/test_monitor_cpu.py) with exact equality, the monitored iteration, RunState with a monitor, and sample_log end to end."""
import functools
import math
import re

import numpy as np
import pytest
import torch

from tests import rig
from tests.test_monitor_cpu import compat_grid

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F32, F64, I64 = np.float32, np.float64, np.int64
GROUP_NAMES = ("idis", "vdis", "gdis")


def _words(t):
    torch.cuda.synchronize()
    return t.cpu().numpy().copy()


def _same_words(got, want, what=""):
    got, want = np.asarray(got, dtype=I64), np.asarray(want, dtype=I64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (what, [(int(i), hex(int(got[i]) & (2 ** 64 - 1)), hex(int(want[i]) & (2 ** 64 - 1))) for i in bad[:8]])


# ---- 1. scalars ---------------------------------------------------------------------------------------------------------------------------------------------------
def _scalar_case():
    g = np.random.default_rng(11)
    v = (g.standard_normal((7, 5)) * 3).astype(F32)
    v[2, 1], v[4, 3], v[0, 2] = np.nan, np.inf, -0.0
    null = {(1, 4), (5, 4)}      # slot 4 is not observed on two of the iterations
    return v, null


def test_scalars_bit_for_bit():
    from dcvgan_amd import monitor as M
    from dcvgan_amd import native
    v, null = _scalar_case()
    names = [f"s{k}" for k in range(5)]
    mon = M.RunMonitor(names, [], device=DEV)
    dev = torch.from_numpy(v).to(DEV)
    w = M.fresh_state(5, 0)
    n0 = native.launch_count()
    for it in range(7):
        mon.observe({names[k]: dev[it, k] for k in range(5) if (it, k) not in null})
        M.monitor_host(w, 5, 0, [None if (it, k) in null else v[it, k] for k in range(5)])
    assert native.launch_count() - n0 == 7
    got = _words(mon.state)
    _same_words(got, w, "window")
    f = got.view(F64)
    o = lambda s, k: M.HEADER_WORDS + s * M.SLOT_WORDS + k
    assert got[M.OBSERVATIONS] == 7 and got[o(4, M.SLOT_COUNT)] == 5 and got[o(1, M.SLOT_NONFINITE)] == 1 and got[o(3, M.SLOT_NONFINITE)] == 1
    assert got[o(1, M.SLOT_COUNT)] == 6 and math.isfinite(f[o(1, M.SLOT_SUM)]) and math.isfinite(f[o(3, M.SLOT_MAX)])      # NaN and inf stayed out of sum and max
    assert f[o(0, M.SLOT_LAST)] == float(v[6, 0]) and f[o(0, M.SLOT_MIN)] == float(v[:, 0].min()) and f[o(0, M.SLOT_MAX)] == float(v[:, 0].max())


def test_integer_valued_scalars_give_the_reference_loggers_mean():
    """logger.py:144-148: avg = sum / count; on small integers and dyadic fractions no order of addition rounds."""
    from dcvgan_amd import monitor as M
    g = np.random.default_rng(12)
    series = [[float(x) for x in g.integers(-100, 101, size=9)], [float(x) / 64.0 for x in g.integers(-999, 1000, size=9)]]
    mon = M.RunMonitor(["a", "b"], [], device=DEV, ring=1)
    dev = torch.tensor(series, dtype=torch.float32).to(DEV)
    for it in range(9):
        mon.observe({"a": dev[0, it], "b": dev[1, it]})
    mon.roll(9)
    (rec,) = mon.drain()
    for name, s in zip("ab", series):
        r = rec["slots"][name]
        assert r["mean"] == sum(s) / len(s) and (r["count"], r["nonfinite"], r["min"], r["max"], r["last"]) == (9, 0, min(s), max(s), s[-1])
    assert (rec["first_iteration"], rec["last_iteration"], rec["observations"], rec["rolls"]) == (1, 9, 9, 0)


# ---- 2. logits ----------------------------------------------------------------------------------------------------------------------------------------------------
LOGIT_SIZES = (1, 2, 255, 256, 257, 513, 4099)


def _logit_case(seed):
    g = np.random.default_rng(seed)
    ys = []
    for n in LOGIT_SIZES:
        y = (g.standard_normal(n) * 2).astype(F32)
        if n >= 255:      # planted: +-0, NaN, +-inf, spread over the lanes and the rows
            y[[0, 7, 100, 254, n - 1, n // 2, 31]] = [0.0, -0.0, np.nan, np.inf, -np.inf, np.nan, -0.0]
        elif n == 2:
            y[:] = [-0.0, np.inf] if seed % 2 else [np.nan, 0.0]
        ys.append(y)
    ys.append(-np.abs(g.standard_normal(300)).astype(F32) - F32(0.5))      # all negative
    return ys


def test_logits_bit_for_bit():
    from dcvgan_amd import monitor as M
    from dcvgan_amd import native
    names = [f"g{n}" for n in LOGIT_SIZES] + ["neg"]
    mon = M.RunMonitor(["s"], names, device=DEV)
    w = M.fresh_state(1, len(names))
    batches = [_logit_case(21), _logit_case(22)]
    n0 = native.launch_count()
    for ys in batches:      # two observations into the same window
        devs = [torch.from_numpy(y).to(DEV) for y in ys]
        mon.observe({}, dict(zip(names, devs)))
        M.monitor_host(w, 1, len(names), None, ys)
    assert native.launch_count() - n0 == 2
    got = _words(mon.state)
    _same_words(got, w, "window")
    for gi, name in enumerate(names):      # the integer fields against plain numpy counts
        o = M.HEADER_WORDS + M.SLOT_WORDS + gi * M.GROUP_WORDS
        both = np.concatenate([b[gi] for b in batches])
        ok = np.isfinite(both)
        assert got[o + M.GROUP_N] == both.size and got[o + M.GROUP_NONFINITE] == np.count_nonzero(~ok), name
        assert got[o + M.GROUP_POS] == np.count_nonzero(both[ok] > 0) and got[o + M.GROUP_NEG] == np.count_nonzero(both[ok] < 0), name
        assert math.isfinite(got.view(F64)[o + M.GROUP_SUM]) and math.isfinite(got.view(F64)[o + M.GROUP_SUMSQ]), name      # NaN and inf stayed out of the sums
    o = M.HEADER_WORDS + M.SLOT_WORDS + (len(names) - 1) * M.GROUP_WORDS
    assert got[o + M.GROUP_POS] == 0 and got[o + M.GROUP_NEG] == 600
    # a null group is skipped: only the group given moves
    before = got.copy()
    y = torch.from_numpy(batches[0][3]).to(DEV)
    mon.observe({}, {names[3]: y, names[4]: None})
    M.monitor_host(w, 1, len(names), None, [batches[0][3] if k == 3 else None for k in range(len(names))])
    after = _words(mon.state)
    _same_words(after, w, "window after a partial observe")
    changed = set(np.nonzero(after != before)[0].tolist())
    o3 = M.HEADER_WORDS + M.SLOT_WORDS + 3 * M.GROUP_WORDS
    assert changed and changed <= {M.OBSERVATIONS} | set(range(o3, o3 + M.GROUP_WORDS))
    # refusals of the Python layer come before any launch
    n0 = native.launch_count()
    for bad, match in ((torch.zeros(4), "HIP device tensor"), (torch.zeros(4, dtype=torch.float16, device=DEV), "float32"),
                       (torch.zeros((4, 2), device=DEV)[:, 0], "contiguous"), (torch.zeros(0, device=DEV), "2\\^24")):
        with pytest.raises(M.NativeError, match=match):
            mon.observe({}, {names[0]: bad})
    with pytest.raises(M.NativeError, match="sync_losses"):
        mon.observe({"s": 0.5})
    with pytest.raises(M.NativeError, match="unknown logit groups"):
        mon.observe({}, {"nope": y})
    assert native.launch_count() == n0
    _same_words(_words(mon.state), w, "window after refusals")


# ---- 3. roll ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_roll_publishes_resets_and_keeps_order():
    from dcvgan_amd import monitor as M
    names, groups = ["a", "b"], ["g"]
    mon = M.RunMonitor(names, groups, device=DEV, ring=2)
    w = M.fresh_state(2, 1)
    g = np.random.default_rng(31)
    want = []
    it = 0
    for r in range(5):      # five windows of 1 .. 5 observations through a ring of two
        for _ in range(r + 1):
            it += 1
            v = (g.standard_normal(2) * 5).astype(F32)
            y = g.standard_normal(300 + 7 * r).astype(F32)
            dv, dy = torch.from_numpy(v).to(DEV), torch.from_numpy(y).to(DEV)
            mon.observe({"a": dv[0], "b": dv[1] if r != 2 else None}, {"g": dy})
            M.monitor_host(w, 2, 1, [v[0], v[1] if r != 2 else None], [y])
        mon.roll(it)
        want.append(M.monitor_host(w, 2, 1, roll=it))
        if r == 0:      # published, then reset: the live window is a fresh one that starts after the roll
            live = _words(mon.state)
            _same_words(live, w, "window after the first roll")
            fresh = M.fresh_state(2, 1, first_iteration=it + 1)
            fresh[M.LAST_ITERATION], fresh[M.ROLLS] = it, 1
            _same_words(live, fresh, "reset window")
    assert mon.rolled == 5
    recs = mon.drain()
    assert len(recs) == 5 and mon.drain() == [] and mon.poll() == []
    first = 1
    for r, (rec, words) in enumerate(zip(recs, want)):
        _same_words(rec["words"], words, f"record {r}")
        assert (rec["first_iteration"], rec["last_iteration"], rec["observations"], rec["rolls"]) == (first, first + r, r + 1, r)
        assert rec["slots"]["a"]["count"] == r + 1 and rec["slots"]["b"]["count"] == (0 if r == 2 else r + 1) and rec["groups"]["g"]["n"] == (r + 1) * (300 + 7 * r)
        first += r + 1
    assert math.isnan(recs[2]["slots"]["b"]["mean"]) and recs[2]["slots"]["b"]["min"] == math.inf      # the second window is independent of the first
    assert recs[1]["slots"]["a"]["min"] != recs[0]["slots"]["a"]["min"] or recs[1]["slots"]["a"]["max"] != recs[0]["slots"]["a"]["max"]


def test_no_host_read_no_torch_kernel():
    """observe, roll and poll under torch's sync debug mode, by the library's launch counter, and under the profiler."""
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    from dcvgan_amd import monitor as M
    from dcvgan_amd import native
    mon = M.RunMonitor(["a", "b"], ["g", "h"], device=DEV, ring=2)
    v = torch.tensor([1.5, -2.0]).to(DEV)
    y = torch.arange(-300, 700, dtype=torch.float32).to(DEV)
    out, logits = {"a": v[0], "b": v[1]}, {"g": y, "h": None}
    for it in (1, 2):      # warm-up: the ring's records, their pinned twins and the side stream are made here
        mon.observe(out, logits)
        mon.roll(it)
    assert len(mon.drain()) == 2
    torch.cuda.synchronize()
    got, deltas = [], []
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        torch.cuda.set_sync_debug_mode("error")
        try:
            for it in (3, 4, 5, 6, 7):      # five rolls through a ring of two: the ring's one wait is an event's, which reads nothing
                n0 = native.launch_count()
                mon.observe(out, logits)
                n1 = native.launch_count()
                mon.roll(it)
                n2 = native.launch_count()
                got += mon.poll()
                deltas.append((n1 - n0, n2 - n1, native.launch_count() - n2))
        finally:
            torch.cuda.set_sync_debug_mode("default")
        got += mon.drain()
        torch.cuda.synchronize()
    assert deltas == [(1, 1, 0)] * 5, deltas      # observe: one launch; roll: one; poll: none
    kernels = {e.key: e.count for e in prof.key_averages() if e.device_type == DeviceType.CUDA}
    foreign = {k[:160]: n for k, n in kernels.items() if "at::" in k or "torch" in k.lower()}
    assert not foreign, foreign
    mine = {k[:60]: n for k, n in kernels.items() if "monitor_" in k}
    assert sorted(mine.values()) == [5, 5] and any("monitor_observe" in k for k in mine) and any("monitor_roll" in k for k in mine), kernels
    assert [r["last_iteration"] for r in got] == [3, 4, 5, 6, 7] and all(r["observations"] == 1 and r["groups"]["g"]["pos"] == 699 for r in got)
    assert all(r["groups"]["g"]["mean"] == 199.5 and r["groups"]["h"]["n"] == 0 and r["slots"]["b"]["mean"] == -2.0 for r in got)


# ---- 4. the iteration ---------------------------------------------------------------------------------------------------------------------------------------------
def _runner(monitor, seed=21, guard=None, lecam_kw=None, interval=2, **cfg_kw):
    from dcvgan_amd import native, trainer
    native.lib()
    cfg = rig.small_cfg(**cfg_kw)
    models, _ = rig.seeded_models(cfg, DEV, seed, 9)
    opts = trainer.build_optimizers(cfg, models, guard=guard)
    lc = trainer.build_lecam(cfg, models, opts, **lecam_kw) if lecam_kw is not None else None
    mon = trainer.build_monitor(cfg, models, opts, interval=interval, lecam=lc) if monitor else None
    kw = dict(monitor=mon) if monitor else {}
    runner = trainer.StepRunner(cfg, models, opts, trainer.build_loss(cfg), lecam=lc, **kw)
    return dict(cfg=cfg, models=models, opts=opts, lc=lc, mon=mon, runner=runner)


def _data(cfg):
    return rig.clip_pair(cfg, DEV, 4)


_model_bytes = rig.state_bytes
# the library's launches per iteration; from the second iteration on (the first makes optimiser state, workspaces and pointer tables) no host sync is allowed
_counted_steps = functools.partial(rig.counted_steps, strict_from=1)


def _hook_logits(models):
    """Forward hooks on the three discriminators: clones of every output, in call order (per iteration: real, the D phase's fakes, the G phase's)."""
    seen = {n: [] for n in GROUP_NAMES}
    handles = [models[n].register_forward_hook(lambda m, i, o, n=n: seen[n].append(o.detach().clone())) for n in GROUP_NAMES]
    return seen, handles


def _mirror_records(run, outs, seen, interval, gated=lambda it: ()):
    """The records the monitor must publish, from the per-iteration results and the hooked logits."""
    from dcvgan_amd import monitor as M
    mon = run["mon"]
    torch.cuda.synchronize()
    w = M.fresh_state(len(mon.slots), len(mon.groups))
    records = []
    for it, out in enumerate(outs, start=1):
        scalars = [None if name in gated(it) else float(out[name]) for name in mon.slots]
        logits = []
        for group in mon.groups:
            n, kind = group.split("_", 1)
            logits.append(seen[n][3 * (it - 1) + ("real", "fake_d", "fake_g").index(kind)].cpu().numpy())
        M.monitor_host(w, len(mon.slots), len(mon.groups), scalars, logits)
        if it % interval == 0:
            records.append(M.monitor_host(w, len(mon.slots), len(mon.groups), roll=it))
    return records, w


def _bits(out):
    return {k: np.array([float(v)], dtype=F32).view(np.uint32)[0] for k, v in out.items()}


def _iteration(guard, lecam_kw, **cfg_kw):
    ts = [2, 3, 4, 5]
    plain = _runner(False, guard=guard, lecam_kw=lecam_kw, **cfg_kw)
    xc, xg = _data(plain["cfg"])
    p_counts, p_outs = _counted_steps(plain["runner"], xc, xg, ts)
    p_bytes = _model_bytes(plain["models"])
    run = _runner(True, guard=guard, lecam_kw=lecam_kw, **cfg_kw)
    seen, handles = _hook_logits(run["models"])
    m_counts, m_outs = _counted_steps(run["runner"], xc, xg, ts)
    for h in handles:
        h.remove()
    m_bytes = _model_bytes(run["models"])
    # the monitor only reads: every parameter, BatchNorm buffer and returned value is the plain run's
    assert p_bytes.keys() == m_bytes.keys() and len(p_bytes) > 100 and all(torch.equal(p_bytes[k], m_bytes[k]) for k in p_bytes)
    assert [_bits(o) for o in p_outs] == [_bits(o) for o in m_outs] and all(set(o) >= {"loss_idis", "loss_vdis", "loss_gdis", "loss_gen"} for o in m_outs)
    # one launch more per iteration, and one more on the iterations that roll
    extra = [m - p for m, p in zip(m_counts, p_counts)]
    print(f"\n[monitor iteration] launches per iteration {m_counts} vs plain {p_counts}: extra {extra}; slots {run['mon'].slots}")
    assert extra == [1, 2, 1, 2]
    assert all(len(v) == 12 for v in seen.values())
    return run, m_outs, seen


def test_iteration():
    """4 iterations, interval 2, with and without the monitor: bit-identical runs, the two records equal the mirror, 1 (+1) extra launches."""
    from dcvgan_amd import trainer
    run, outs, seen = _iteration(None, None)
    mon = run["mon"]
    assert mon.slots == ("loss_idis", "loss_vdis", "loss_gdis", "loss_gen") and mon.groups == trainer.MONITOR_GROUPS
    want, w = _mirror_records(run, outs, seen, 2)
    recs = mon.drain()
    assert len(recs) == len(want) == 2 and [(r["first_iteration"], r["last_iteration"], r["observations"], r["rolls"]) for r in recs] == [(1, 2, 2, 0), (3, 4, 2, 1)]
    for k, (rec, words) in enumerate(zip(recs, want)):
        _same_words(rec["words"], words, f"record {k}")
        assert all(s["count"] == 2 and s["nonfinite"] == 0 and math.isfinite(s["mean"]) for s in rec["slots"].values())
        assert all(g["n"] > 0 and g["nonfinite"] == 0 and g["pos"] + g["neg"] <= g["n"] and 0.0 <= g["frac_pos"] <= 1.0 for g in rec["groups"].values())
        assert rec["slots"]["loss_gen"]["last"] == float(outs[2 * k + 1]["loss_gen"])
    _same_words(_words(mon.state), w, "live window")


def test_iteration_with_guard_and_lecam_and_a_gated_phase():
    """The extra slots in the stated order; with num_gen_update = 2 the D phase steps on even iterations only: its guard slots are not observed on the odd ones."""
    run, outs, seen = _iteration(dict(max_norm=10.0), dict(weight=0.3, start=0, one_sided=False), num_gen_update=2)
    mon = run["mon"]
    assert mon.slots == ("loss_idis", "loss_vdis", "loss_gdis", "loss_gen", "lecam_idis", "lecam_vdis", "lecam_gdis", "grad_norm_dis", "skipped_dis", "grad_norm_gen",
                         "skipped_gen")
    gated = lambda it: ("grad_norm_dis", "skipped_dis") if it % 2 else ()
    want, w = _mirror_records(run, outs, seen, 2, gated)
    recs = mon.drain()
    assert len(recs) == 2
    for k, (rec, words) in enumerate(zip(recs, want)):
        _same_words(rec["words"], words, f"record {k}")
        assert rec["slots"]["grad_norm_dis"]["count"] == rec["slots"]["skipped_dis"]["count"] == 1      # the gated iteration left them alone
        assert rec["slots"]["grad_norm_gen"]["count"] == 2 and rec["slots"]["lecam_vdis"]["count"] == 2 and rec["slots"]["grad_norm_dis"]["mean"] > 0
    _same_words(_words(mon.state), w, "live window")


# ---- 5. RunState --------------------------------------------------------------------------------------------------------------------------------------------------
def test_run_state_carries_the_window(tmp_path):
    from dcvgan_amd import runstate, trainer
    run = _runner(True, interval=4)
    cfg, mon, runner = run["cfg"], run["mon"], run["runner"]
    xc, xg = _data(cfg)
    rs = trainer.build_run_state(cfg, run["models"], run["opts"], runner=runner, monitor=mon)
    assert rs.manifest()[-1]["name"] == "monitor.state"
    runner.step(xc, xg, 2)
    runner.step(xc, xg, 3)
    snap = rs.capture()      # mid-window
    path = str(tmp_path / "run.pt")
    snap.save(path)
    at_capture = _words(mon.state)
    assert at_capture[2] == 2 and snap.host["monitor"]["rolled"] == 0 and snap.host["iteration"] == 2
    runner.step(xc, xg, 4)
    assert _words(mon.state)[2] == 3
    snap.restore()
    _same_words(_words(mon.state), at_capture, "restored window")
    runner.step(xc, xg, 4)
    runner.step(xc, xg, 5)      # iteration 4: the roll
    (first,) = mon.drain()
    assert (first["first_iteration"], first["last_iteration"], first["observations"]) == (1, 4, 4)
    # the same from the file, in fresh objects built with a monitor
    run2 = _runner(True, seed=77, interval=9)
    rs2 = trainer.build_run_state(cfg, run2["models"], run2["opts"], runner=run2["runner"], monitor=run2["mon"])
    rs2.load(path).restore()
    assert run2["mon"].interval == 4 and run2["runner"].iteration == 2
    _same_words(_words(run2["mon"].state), at_capture, "loaded window")
    run2["runner"].step(xc, xg, 4)
    run2["runner"].step(xc, xg, 5)
    (second,) = run2["mon"].drain()
    _same_words(second["words"], first["words"], "the record after a resume")
    # a monitored snapshot and an unmonitored run (and the other way round) refuse one another, naming the first difference
    bare = trainer.build_run_state(cfg, run2["models"], run2["opts"], runner=run2["runner"])
    with pytest.raises(runstate.NativeError, match="monitor.state: not part of the live state"):
        bare.load(path)
    bare_path = str(tmp_path / "bare.pt")
    bare.capture().save(bare_path)
    with pytest.raises(runstate.NativeError, match="monitor.state: not part of the snapshot"):
        rs2.load(bare_path)
    with pytest.raises(runstate.NativeError, match="monitor.state: not part of the live state"):
        trainer.build_run_state(cfg, run["models"], run["opts"], runner=runner)._check(snap.manifest, snap.host)


# ---- 6. the histogram ---------------------------------------------------------------------------------------------------------------------------------------------
def _hist(x, channel=0, counts=None, accumulate=False):
    from dcvgan_amd import monitor as M
    return M.hist_u8(x, channel, counts, accumulate)


@pytest.mark.parametrize("shape,channel", [((3, 3, 2, 5, 7), 0), ((3, 3, 2, 5, 7), 2), ((1, 1, 1, 1, 1), 0), ((2, 1, 16, 64, 64), 0), ((2, 3, 1, 4, 16), 1),
                                           ((1, 2, 3, 37, 449), 1)])
def test_histogram_is_bincount(shape, channel):
    """(3,3,2,5,7): runs of 70 bytes at stride 210, misaligned starts; (2,1,16,64,64): several workgroups; (1,2,3,37,449): a run of 49839 bytes that starts at an
    odd address and ends in a partial chunk."""
    from dcvgan_amd import monitor as M
    from dcvgan_amd import native
    g = np.random.default_rng(sum(shape))
    x = g.integers(0, 256, size=shape, dtype=np.uint8)
    dx = torch.from_numpy(x).to(DEV)
    n0 = native.launch_count()
    counts = _hist(dx, channel)
    assert native.launch_count() - n0 == 2      # the zeroing and the counting
    got = _words(counts)
    want = np.bincount(x[:, channel].ravel(), minlength=256)
    assert counts.dtype == torch.int64 and np.array_equal(got, want) and np.array_equal(got, M.hist_host(x, channel))
    assert got.sum() == x[:, channel].size


def test_histogram_contention_accumulate_and_overwrite():
    from dcvgan_amd import native
    shape = (2, 1, 16, 64, 64)
    x = torch.full(shape, 255, dtype=torch.uint8).to(DEV)      # every byte in one bin: a depth clip's background
    got = _words(_hist(x))
    assert got[255] == 2 * 16 * 64 * 64 and got.sum() == got[255]
    g = np.random.default_rng(61)
    a = g.integers(0, 256, size=(3, 3, 2, 5, 7), dtype=np.uint8)
    b = np.minimum(g.integers(0, 256, size=(2, 3, 1, 4, 16)), 3).astype(np.uint8)      # few bins: long equal runs inside a vector
    counts = torch.from_numpy(np.full(256, 0x7FF8000000000001, dtype=I64)).to(DEV)      # a NaN's bits: accumulate = 0 overwrites them
    _hist(torch.from_numpy(a).to(DEV), 0, counts)
    first = _words(counts)
    assert np.array_equal(first, np.bincount(a[:, 0].ravel(), minlength=256))
    n0 = native.launch_count()
    _hist(torch.from_numpy(b).to(DEV), 0, counts, accumulate=True)
    assert native.launch_count() - n0 == 1
    assert np.array_equal(_words(counts), first + np.bincount(b[:, 0].ravel(), minlength=256))
    # a view that starts one byte off a 16-byte boundary
    flat = torch.from_numpy(g.integers(0, 256, size=1 + 2 * 2 * 3 * 8 * 16, dtype=np.uint8)).to(DEV)
    v = flat[1:].view(2, 2, 3, 8, 16)
    assert v.data_ptr() % 16 == 1
    assert np.array_equal(_words(_hist(v, 1)), np.bincount(v.cpu().numpy()[:, 1].ravel(), minlength=256))


# ---- 7. the grid --------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols,thw", [(2, 3, (3, 5, 7)), (1, 1, (1, 1, 1)), (2, 2, (2, 4, 16)), (2, 2, (2, 4, 32)), (3, 2, (2, 3, 48))])
def test_grid_is_the_compat_route(rows, cols, thw):
    from dcvgan_amd import monitor as M
    from dcvgan_amd import native
    g = np.random.default_rng(rows * 100 + cols * 10 + thw[2])
    geo = g.integers(0, 256, size=(rows * cols, 3) + thw, dtype=np.uint8)
    col = g.integers(0, 256, size=(rows * cols, 3) + thw, dtype=np.uint8)
    n0 = native.launch_count()
    out = M.video_grid_u8(torch.from_numpy(geo).to(DEV), torch.from_numpy(col).to(DEV), rows, cols)
    assert native.launch_count() - n0 == 1
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert got.shape == (1, thw[0], 3, rows * thw[1], 2 * cols * thw[2]) and got.dtype == np.uint8
    assert np.array_equal(got, compat_grid(geo, col, rows, cols)) and np.array_equal(got, M.grid_host(geo, col, rows, cols))


def test_grid_with_a_misaligned_input_takes_the_bytewise_path():
    from dcvgan_amd import monitor as M
    g = np.random.default_rng(71)
    shape = (4, 3, 2, 4, 16)
    n = int(np.prod(shape))
    geo = g.integers(0, 256, size=shape, dtype=np.uint8)
    col = g.integers(0, 256, size=shape, dtype=np.uint8)
    flat = torch.zeros(n + 1, dtype=torch.uint8).to(DEV)
    off = flat[1:].view(shape)
    off.copy_(torch.from_numpy(geo))
    assert off.data_ptr() % 16 == 1 and off.is_contiguous()
    dcol = torch.from_numpy(col).to(DEV)
    want = compat_grid(geo, col, 2, 2)
    torch.cuda.synchronize()
    assert np.array_equal(M.video_grid_u8(off, dcol, 2, 2).cpu().numpy(), want)
    assert np.array_equal(M.video_grid_u8(dcol, off, 2, 2).cpu().numpy(), compat_grid(col, geo, 2, 2))
    with pytest.raises(M.NativeError, match="do not fill"):
        M.video_grid_u8(dcol, dcol, 3, 2)
    with pytest.raises(M.NativeError, match="contiguous"):
        M.video_grid_u8(dcol.transpose(3, 4), dcol.transpose(3, 4), 2, 2)


# ---- 8. sample_log ------------------------------------------------------------------------------------------------------------------------------------------------
def _generators(kind):
    from dcvgan_amd import generator, util
    torch.manual_seed(5)
    ch = {"depth": 1, "optical-flow": 2}[kind]
    ggen = generator.GeometricVideoGenerator(dim_z_content=30, dim_z_motion=10, channel=ch, geometric_info=kind, video_length=16, ngf=8).to(DEV)
    cgen = generator.ColorVideoGenerator(in_ch=ch, dim_z=10, geometric_info=kind, ngf=8).to(DEV)
    for m in (ggen, cgen):
        m.apply(util.init_weights)
    return ggen, cgen


def _seed(ggen, cgen):
    from dcvgan_amd.rng import PhiloxRng
    ggen._rng, cgen._rng = PhiloxRng(41), PhiloxRng(42)


def _host_route(xg, xc, rows, cols):
    return dict(video=compat_grid(xg, xc, rows, cols), hist_geo=np.bincount(xg[:, 0].ravel(), minlength=256), hist_colour=np.bincount(xc[:, 0].ravel(), minlength=256))


def _same_log(got, want):
    assert set(got) == {"video", "hist_geo", "hist_colour"}
    assert got["video"].dtype == np.uint8 and got["hist_geo"].dtype == got["hist_colour"].dtype == I64
    for k in want:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k


@pytest.mark.parametrize("kind", ["depth", "optical-flow"])
def test_sample_log_end_to_end(kind):
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    from dcvgan_amd import monitor as M
    from dcvgan_amd import native, sampling
    native.lib()
    ggen, cgen = _generators(kind)
    rows = cols = 2
    _seed(ggen, cgen)
    xg, xc = sampling.generate_samples(ggen, cgen, 4, 4)
    want = _host_route(xg, xc, rows, cols)
    _seed(ggen, cgen)
    M.sample_log(ggen, cgen, 4, rows, cols)      # warm-up: workspaces
    _seed(ggen, cgen)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        got = M.sample_log(ggen, cgen, 4, rows, cols)
        torch.cuda.synchronize()
    _same_log(got, want)
    assert got["video"].shape == (1, 16, 3, 2 * 64, 4 * 64) and got["hist_geo"].sum() == got["hist_colour"].sum() == 4 * 16 * 64 * 64
    events = {e.key: e.count for e in prof.key_averages() if e.device_type == DeviceType.CUDA}
    foreign = {k[:160]: n for k, n in events.items() if "at::" in k or "torch" in k.lower()}
    assert not foreign, foreign
    copies = {k: n for k, n in events.items() if re.search(r"(?i)memcpy|copy", k) and not re.search(r"(?i)kernel", k)}
    d2h = {k: n for k, n in copies.items() if re.search(r"(?i)dtoh|device\s*->\s*(host|pageable|pinned)|devicetohost", k)}
    print(f"\n[sample_log {kind}] copies under the profiler: {copies}")
    assert sum(d2h.values()) == 3, (copies, sorted(events))      # the grid and the two count vectors
    # batches of 3: the second is truncated to one clip, as generate_samples truncates it
    _seed(ggen, cgen)
    xg3, xc3 = sampling.generate_samples(ggen, cgen, 4, 3)
    _seed(ggen, cgen)
    _same_log(M.sample_log(ggen, cgen, 4, rows, cols, batchsize=3), _host_route(xg3, xc3, rows, cols))
    # a real batch (trainer.py:146-169): its first four clips
    g = torch.Generator().manual_seed(9)
    rg = torch.rand(5, 1 if kind == "depth" else 2, 4, 8, 16, generator=g) * 2.4 - 1.2
    rc = torch.rand(5, 3, 4, 8, 16, generator=g) * 2.4 - 1.2
    drg, drc = rg.to(DEV), rc.to(DEV)
    want_real = _host_route(sampling.geometry_to_color(drg[:4], kind), sampling.videos_to_numpy(drc[:4]), 1, 4)
    _same_log(M.sample_log(ggen, cgen, 4, 1, 4, real=(drg, drc)), want_real)
