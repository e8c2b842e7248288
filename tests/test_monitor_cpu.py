"""CPU: RunMonitor's binding, the entry points' refusals, the numpy mirrors of the four kernels and the wiring into StepRunner / RunState.

`monitor_host`, `hist_host` and `grid_host` are the specifications tests/test_monitor_gpu.py holds the kernels to; here they are checked against Python's own
arithmetic, numpy's bincount and the reference's make_video_grid route."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import rig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dcv_monitor_observe", "dcv_monitor_roll", "dcv_hist_u8", "dcv_video_grid_u8")
CPU = torch.device("cpu")
F32, F64, I64 = np.float32, np.float64, np.int64


# ---- the binding ------------------------------------------------------------------------------------------------------------------------------------------------
def test_new_names_are_bound_declared_and_exported():
    from dcvgan_amd import monitor as M
    from dcvgan_amd import native
    if not os.path.exists(native.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    text = open(os.path.join(ROOT, "include", "dcvgan_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    raw = ctypes.CDLL(native.LIB_PATH)
    for n in NEW:
        assert n in native.EXPORTS, n
        assert re.search(r"\b%s\s*\(" % n, header), f"{n} is not declared in dcvgan_hip.h"
        assert hasattr(raw, n), f"{n} is not exported by the library"
    declared = set(re.findall(r"\b(dcv_\w+)\s*\(", header))
    assert declared == set(native.EXPORTS), declared ^ set(native.EXPORTS)
    build = open(os.path.join(ROOT, "dcvgan_amd", "csrc", "build.sh")).read()
    assert re.search(r"for f in [^;]*\bmonitor\b", build) and "$OBJ/monitor.o" in build
    assert native.lib().dcv_version() == native.ABI_VERSION == 4
    # the word counts of the header are the module's
    defs = dict(re.findall(r"#define (DCV_MONITOR_\w+) (\d+)", text))
    assert int(defs["DCV_MONITOR_HEADER_WORDS"]) == M.HEADER_WORDS == 4 and int(defs["DCV_MONITOR_SLOT_WORDS"]) == M.SLOT_WORDS == 6
    assert int(defs["DCV_MONITOR_GROUP_WORDS"]) == M.GROUP_WORDS == 6
    assert int(defs["DCV_MONITOR_MAX_SLOTS"]) == M.MAX_SLOTS == 32 and int(defs["DCV_MONITOR_MAX_GROUPS"]) == M.MAX_GROUPS == 16
    for name in ("FIRST_ITERATION", "LAST_ITERATION", "OBSERVATIONS", "ROLLS", "SLOT_SUM", "SLOT_COUNT", "SLOT_NONFINITE", "SLOT_MIN", "SLOT_MAX", "SLOT_LAST",
                 "GROUP_N", "GROUP_SUM", "GROUP_SUMSQ", "GROUP_POS", "GROUP_NEG", "GROUP_NONFINITE"):
        assert int(defs["DCV_MONITOR_" + name]) == getattr(M, name), name


def test_entry_points_refuse_before_any_launch():
    """No GPU is needed to be refused."""
    from dcvgan_amd import native
    L = native.lib()
    i64 = lambda xs: (ctypes.c_int64 * len(xs))(*xs)
    vp = lambda xs: (ctypes.c_void_p * len(xs))(*xs)
    P = ctypes.c_void_p
    n0 = native.launch_count()
    EINVAL = native.DCV_EINVAL
    slots, groups, ns, state, record = vp([0x1000, 0]), vp([0x2000, 0]), i64([5, 0]), P(0x10000), P(0x20000)
    # observe
    assert L.dcv_monitor_observe(33, vp([0x1000] * 33), 0, None, None, state, None) == EINVAL and b"n_slots" in L.dcv_last_error()
    assert L.dcv_monitor_observe(0, None, 17, vp([0x1000] * 17), i64([1] * 17), state, None) == EINVAL and b"n_groups" in L.dcv_last_error()
    assert L.dcv_monitor_observe(-1, slots, 2, groups, ns, state, None) == EINVAL
    assert L.dcv_monitor_observe(2, None, 2, groups, ns, state, None) == EINVAL and b"null table" in L.dcv_last_error()
    assert L.dcv_monitor_observe(2, slots, 2, None, ns, state, None) == EINVAL
    assert L.dcv_monitor_observe(2, slots, 2, groups, None, state, None) == EINVAL
    assert L.dcv_monitor_observe(2, slots, 2, groups, ns, None, None) == EINVAL
    assert L.dcv_monitor_observe(2, slots, 2, groups, ns, P(0x10004), None) == EINVAL and b"8-byte" in L.dcv_last_error()
    for bad in (0, -3, (1 << 24) + 1):
        assert L.dcv_monitor_observe(2, slots, 2, groups, i64([bad, 0]), state, None) == EINVAL and b"2^24" in L.dcv_last_error()
    assert L.dcv_monitor_observe(2, vp([0x1002, 0]), 2, groups, ns, state, None) == EINVAL
    assert L.dcv_monitor_observe(2, slots, 2, vp([0x2001, 0]), ns, state, None) == EINVAL
    # roll
    assert L.dcv_monitor_roll(33, 0, state, record, 1, None) == EINVAL and L.dcv_monitor_roll(0, 17, state, record, 1, None) == EINVAL
    assert L.dcv_monitor_roll(2, 2, None, record, 1, None) == EINVAL and L.dcv_monitor_roll(2, 2, state, None, 1, None) == EINVAL
    assert L.dcv_monitor_roll(2, 2, P(0x10004), record, 1, None) == EINVAL and L.dcv_monitor_roll(2, 2, state, P(0x20004), 1, None) == EINVAL
    assert L.dcv_monitor_roll(2, 2, state, state, 1, None) == EINVAL
    # histogram
    x, counts = P(0x30000), P(0x40000)
    assert L.dcv_hist_u8(x, 2, 3, 4, 5, 6, 3, counts, 0, None) == EINVAL and b"channel" in L.dcv_last_error()      # a channel index >= C
    assert L.dcv_hist_u8(x, 2, 3, 4, 5, 6, -1, counts, 0, None) == EINVAL
    assert L.dcv_hist_u8(x, 0, 3, 4, 5, 6, 0, counts, 0, None) == EINVAL and L.dcv_hist_u8(x, 2, 3, 4, 5, 0, 0, counts, 0, None) == EINVAL
    assert L.dcv_hist_u8(None, 2, 3, 4, 5, 6, 0, counts, 0, None) == EINVAL
    assert L.dcv_hist_u8(x, 2, 3, 4, 5, 6, 0, None, 0, None) == EINVAL and L.dcv_hist_u8(x, 2, 3, 4, 5, 6, 0, P(0x40004), 1, None) == EINVAL
    # grid
    g, c, out = P(0x50000), P(0x60000), P(0x70000)
    assert L.dcv_video_grid_u8(g, c, 2, 3, 5, 4, 5, 6, out, None) == EINVAL and b"do not fill" in L.dcv_last_error()      # rows * cols != N
    assert L.dcv_video_grid_u8(g, c, 0, 3, 0, 4, 5, 6, out, None) == EINVAL and L.dcv_video_grid_u8(g, c, 2, 3, 6, 4, 0, 6, out, None) == EINVAL
    assert L.dcv_video_grid_u8(None, c, 2, 3, 6, 4, 5, 6, out, None) == EINVAL and L.dcv_video_grid_u8(g, None, 2, 3, 6, 4, 5, 6, out, None) == EINVAL
    assert L.dcv_video_grid_u8(g, c, 2, 3, 6, 4, 5, 6, None, None) == EINVAL
    assert native.launch_count() == n0


# ---- the mirrors ------------------------------------------------------------------------------------------------------------------------------------------------
def test_window_mean_is_the_reference_loggers_on_exact_values():
    """Loss.update / Loss.avg of the reference's logger (logger.py:144-148): sum of the values over their number.  On dyadic and small-integer values every order
    of summation is exact, so the window's sum / count must equal Python's sum(v) / len(v) bit for bit."""
    from dcvgan_amd import monitor as M
    g = np.random.default_rng(5)
    series = [[float(v) for v in g.integers(-100, 101, size=37)], [float(v) / 256.0 for v in g.integers(-4095, 4096, size=100)], [0.5], [3.0, -3.0, 0.25]]
    n = len(series)
    w = M.fresh_state(n, 0)
    for it in range(max(len(s) for s in series)):
        M.monitor_host(w, n, 0, [s[it] if it < len(s) else None for s in series])
    rec = M.parse_record(M.monitor_host(w, n, 0, roll=100), [f"s{k}" for k in range(n)], [])
    assert (rec["first_iteration"], rec["last_iteration"], rec["observations"], rec["rolls"]) == (1, 100, 100, 0)
    for k, s in enumerate(series):
        r = rec["slots"][f"s{k}"]
        assert r["mean"] == sum(s) / len(s) and r["count"] == len(s) and r["nonfinite"] == 0
        assert (r["min"], r["max"], r["last"]) == (min(s), max(s), s[-1])
    # the same through a logit group: integers in every lane order
    y = g.integers(-50, 51, size=4099).astype(F32)
    w = M.fresh_state(0, 1)
    M.monitor_host(w, 0, 1, None, [y])
    M.monitor_host(w, 0, 1, None, [y[:300]])
    r = M.parse_record(M.monitor_host(w, 0, 1, roll=2), [], ["g"])["groups"]["g"]
    both = [float(v) for v in y] + [float(v) for v in y[:300]]
    assert r["n"] == len(both) and r["mean"] == sum(both) / len(both)
    assert r["pos"] == sum(v > 0 for v in both) and r["neg"] == sum(v < 0 for v in both) and r["frac_pos"] == r["pos"] / len(both)
    assert r["std"] == math.sqrt(sum(v * v for v in both) / len(both) - r["mean"] ** 2)


def test_mirror_orders_nonfinite_values_zeros_and_the_roll():
    from dcvgan_amd import monitor as M
    # the lane-strided order and the tree, restated one scalar at a time
    g = np.random.default_rng(6)
    for n in (1, 2, 255, 256, 257, 513, 1000):
        v = g.standard_normal(n).astype(F32).astype(F64) * 1e3
        p = [0.0] * 256
        for i in range(n):
            p[i % 256] = p[i % 256] + float(v[i])
        s = 128
        while s >= 1:
            for l in range(s):
                p[l] = p[l] + p[l + s]
            s //= 2
        assert M._lane_tree_sum(v) == p[0], n
    assert M._lane_tree_sum(np.arange(1, 1001, dtype=F64)) == 500500.0
    # non-finite values: counted, kept out of sum / min / max and of the sign counts; last takes everything; +-0 is neither positive nor negative
    w = M.fresh_state(2, 1)
    y = np.array([1.5, -0.0, 0.0, np.nan, np.inf, -np.inf, -2.0, 3.0], dtype=F32)
    for v in (2.0, float("nan"), -0.0, float("inf"), 7.0):
        M.monitor_host(w, 2, 1, [v, None], [y])
    rec = M.parse_record(M.monitor_host(w, 2, 1, roll=5), ["a", "b"], ["g"])
    a, b, grp = rec["slots"]["a"], rec["slots"]["b"], rec["groups"]["g"]
    assert (a["count"], a["nonfinite"], a["mean"], a["min"], a["max"], a["last"]) == (3, 2, 3.0, 0.0, 7.0, 7.0) and math.copysign(1.0, a["min"]) == -1.0
    assert (b["count"], b["nonfinite"], b["min"], b["max"], b["last"]) == (0, 0, math.inf, -math.inf, 0.0) and math.isnan(b["mean"])
    assert (grp["n"], grp["nonfinite"], grp["pos"], grp["neg"]) == (40, 15, 10, 5) and grp["mean"] == 2.5 / 5 and grp["frac_pos"] == 10 / 25
    # the roll: published, then reset; rolls survives and increments; the next window starts after the roll's iteration
    assert (rec["first_iteration"], rec["last_iteration"], rec["observations"], rec["rolls"]) == (1, 5, 5, 0)
    fresh = M.fresh_state(2, 1, first_iteration=6)
    fresh[M.LAST_ITERATION], fresh[M.ROLLS] = 5, 1
    assert np.array_equal(w, fresh)
    M.monitor_host(w, 2, 1, [None, 1.0], None)
    rec2 = M.parse_record(M.monitor_host(w, 2, 1, roll=9), ["a", "b"], ["g"])
    assert (rec2["first_iteration"], rec2["last_iteration"], rec2["observations"], rec2["rolls"]) == (6, 9, 1, 1)
    assert rec2["slots"]["a"]["count"] == 0 and rec2["slots"]["b"]["mean"] == 1.0 and rec2["groups"]["g"]["n"] == 0 and math.isnan(rec2["groups"]["g"]["mean"])


HIST_SHAPES = [((3, 3, 2, 5, 7), 0), ((1, 1, 1, 1, 1), 0), ((2, 3, 1, 4, 16), 1), ((2, 1, 4, 16, 16), 0)]


def test_hist_host_is_bincount():
    from dcvgan_amd import monitor as M
    g = np.random.default_rng(7)
    for shape, ch in HIST_SHAPES:
        x = g.integers(0, 256, size=shape, dtype=np.uint8)
        got = M.hist_host(x, ch)
        assert got.dtype == I64 and got.shape == (256,) and np.array_equal(got, np.bincount(x[:, ch].ravel(), minlength=256))
    x = np.full((2, 2, 2, 3, 3), 255, dtype=np.uint8)
    assert M.hist_host(x, 1)[255] == 36 and M.hist_host(x, 1).sum() == 36


def compat_grid(geo, colour, rows, cols):
    """trainer.py:138-143 of the reference, with compat/util.make_video_grid."""
    from compat import util as CU
    return np.concatenate([CU.make_video_grid(geo, rows, cols), CU.make_video_grid(colour, rows, cols)], axis=-1).transpose(0, 2, 1, 3, 4)


def test_grid_host_is_the_compat_route():
    from dcvgan_amd import monitor as M
    g = np.random.default_rng(8)
    for rows, cols, (t, h, w) in ((2, 3, (3, 5, 7)), (1, 1, (1, 1, 1)), (2, 2, (2, 4, 16)), (3, 1, (2, 2, 3))):
        geo = g.integers(0, 256, size=(rows * cols, 3, t, h, w), dtype=np.uint8)
        col = g.integers(0, 256, size=(rows * cols, 3, t, h, w), dtype=np.uint8)
        got = M.grid_host(geo, col, rows, cols)
        assert got.shape == (1, t, 3, rows * h, 2 * cols * w) and got.dtype == np.uint8
        assert np.array_equal(got, compat_grid(geo, col, rows, cols)), (rows, cols, t, h, w)


# ---- the Python layer -------------------------------------------------------------------------------------------------------------------------------------------
def test_run_monitor_refuses_cpu_tensors_and_bad_arguments():
    from dcvgan_amd import monitor as M
    from dcvgan_amd import native
    n0 = native.launch_count()
    mon = M.RunMonitor(["loss_a", "loss_b"], ["g"], device=CPU, ring=2, interval=5)
    assert mon.state.dtype == torch.int64 and mon.state.numel() == M.state_words(2, 1) == 4 + 12 + 6 and (mon.ring, mon.interval, mon.rolled) == (2, 5, 0)
    assert np.array_equal(mon.state.numpy(), M.fresh_state(2, 1))
    with pytest.raises(M.NativeError, match="GPU only"):
        mon.observe({"loss_a": torch.zeros(())}, {"g": torch.zeros(4)})
    with pytest.raises(M.NativeError, match="GPU only"):
        mon.roll(5)
    assert mon.poll() == [] and mon.drain() == []
    with pytest.raises(ValueError, match="at most 32 slots"):
        M.RunMonitor([f"s{k}" for k in range(33)], [], device=CPU)
    with pytest.raises(ValueError, match="at most 32 slots and 16 groups"):
        M.RunMonitor([], [f"g{k}" for k in range(17)], device=CPU)
    with pytest.raises(ValueError, match="distinct"):
        M.RunMonitor(["a", "a"], [], device=CPU)
    with pytest.raises(ValueError, match="ring"):
        M.RunMonitor(["a"], [], device=CPU, ring=0)
    for t, dtype, match in ((torch.zeros(3), torch.float32, "HIP device tensor"), (0.25, torch.float32, "sync_losses")):
        with pytest.raises(M.NativeError, match=match):
            M._require_cuda(t, "x", dtype)
    with pytest.raises(M.NativeError, match="HIP device tensor"):
        M.hist_u8(torch.zeros((1, 1, 1, 1, 1), dtype=torch.uint8))
    with pytest.raises(M.NativeError, match="HIP device tensor"):
        M.video_grid_u8(torch.zeros((1, 3, 1, 1, 1), dtype=torch.uint8), torch.zeros((1, 3, 1, 1, 1), dtype=torch.uint8), 1, 1)
    with pytest.raises(M.NativeError, match="do not fill"):
        M.sample_log(None, None, 5, 2, 2)
    # the checkpoint conventions of the other components
    sd = mon.state_dict()
    assert sd["slots"] == ["loss_a", "loss_b"] and sd["groups"] == ["g"] and sd["interval"] == 5 and sd["rolled"] == 0 and len(sd["state"]) == 22
    other = M.RunMonitor(["loss_a", "loss_b"], ["g"], device=CPU)
    sd["state"][M.OBSERVATIONS], sd["rolled"] = 3, 7
    other.load_state_dict(sd)
    assert int(other.state[M.OBSERVATIONS]) == 3 and (other.interval, other.rolled) == (5, 7)
    with pytest.raises(ValueError, match="built for slots"):
        M.RunMonitor(["x"], ["g"], device=CPU).load_state_dict(sd)
    assert native.launch_count() == n0


def _host_run(seed, monitor, guard=None, lecam=False):
    from dcvgan_amd import trainer
    cfg = rig.small_cfg()
    models, _ = rig.seeded_models(cfg, CPU, seed, seed + 100)
    opts = trainer.build_optimizers(cfg, models, guard=guard)
    lc = trainer.build_lecam(cfg, models, opts, weight=0.3, start=0) if lecam else None
    mon = trainer.build_monitor(cfg, models, opts, interval=7, lecam=lc, ring=3) if monitor else None
    return cfg, models, opts, lc, mon


def test_build_monitor_takes_its_slots_from_the_run():
    from dcvgan_amd import trainer
    base = ["loss_idis", "loss_vdis", "loss_gdis", "loss_gen"]
    groups = ("idis_real", "idis_fake_d", "idis_fake_g", "vdis_real", "vdis_fake_d", "vdis_fake_g", "gdis_real", "gdis_fake_d", "gdis_fake_g")
    _, _, _, _, mon = _host_run(1, True)
    assert list(mon.slots) == base and mon.groups == groups == trainer.MONITOR_GROUPS and (mon.interval, mon.ring) == (7, 3) and mon.device == CPU
    _, _, _, _, mon = _host_run(1, True, guard=dict(max_norm=10.0), lecam=True)
    assert list(mon.slots) == base + ["lecam_idis", "lecam_vdis", "lecam_gdis", "grad_norm_dis", "skipped_dis", "grad_norm_gen", "skipped_gen"]
    _, _, _, _, mon = _host_run(1, True, guard=dict(max_norm=10.0))
    assert list(mon.slots) == base + ["grad_norm_dis", "skipped_dis", "grad_norm_gen", "skipped_gen"]


def test_step_runner_and_run_state_without_a_monitor_are_unchanged():
    from dcvgan_amd import runstate, trainer
    cfg, models, opts, lc, mon = _host_run(2, True, lecam=True)
    loss = trainer.build_loss(cfg)
    plain = trainer.StepRunner(cfg, models, opts, loss, lecam=lc)
    assert plain.monitor is None and trainer.StepRunner(cfg, models, opts, loss, lecam=lc, monitor=None).monitor is None
    assert trainer.StepRunner(cfg, models, opts, loss, lecam=lc, monitor=mon).monitor is mon
    with pytest.raises(ValueError, match="sync_losses"):
        trainer.StepRunner(cfg, models, opts, loss, lecam=lc, monitor=mon, sync_losses=True)
    # RunState: without a monitor no entry, no key; with one, the window and a block of host scalars
    bare = trainer.build_run_state(cfg, models, opts, runner=plain, lecam=lc)
    assert bare.monitor is None and runstate.RunState(models, opts, runner=plain, lecam=lc, monitor=None).manifest() == bare.manifest()
    assert bare.manifest()[-1]["name"] == "lecam.state" and "monitor" not in bare.capture().host
    with_mon = trainer.build_run_state(cfg, models, opts, runner=plain, lecam=lc, monitor=mon)
    man = with_mon.manifest()
    assert [e["name"] for e in man[:-1]] == [e["name"] for e in bare.manifest()] and man[-1]["name"] == "monitor.state"
    assert man[-1]["dtype"] == "torch.int64" and man[-1]["dwords"] == 2 * mon.words
    mon.rolled = 5
    snap = with_mon.capture()
    assert snap.host["monitor"] == dict(slots=list(mon.slots), groups=list(mon.groups), interval=7, rolled=5)
    # a rollback brings the window's words and the ring position back (host tensors: the numpy mirror of the pack)
    before = mon.state.clone()
    mon.state[3] = 99
    mon.rolled, mon.interval = 8, 50
    snap.restore()
    assert torch.equal(mon.state, before) and (mon.rolled, mon.interval) == (5, 7)
    # the two kinds of run do not take one another's snapshots, and the first difference is named
    with pytest.raises(runstate.NativeError, match="monitor.state: not part of the live state"):
        bare._check(snap.manifest, snap.host)
    with pytest.raises(runstate.NativeError, match="monitor.state: not part of the snapshot"):
        s = bare.capture()
        with_mon._check(s.manifest, s.host)
    _, models2, opts2, lc2, mon2 = _host_run(2, True, guard=dict(max_norm=1.0), lecam=True)      # other slots: another window
    other = trainer.build_run_state(cfg, models2, opts2, runner=plain, lecam=lc2, monitor=mon2)
    with pytest.raises(runstate.NativeError, match="monitor.state"):
        other._check(snap.manifest, snap.host)
