"""CPU: tests/rig.py itself.  The launcher against a stub rank (tests/rig_stub_worker.py: plain Python, exit statuses only, no signal), the fault latch, and the
step rig's seeded models, data pair and launch counter on the host."""
import os
import time

import pytest
import torch

from tests import rig

CPU = torch.device("cpu")


@pytest.fixture(autouse=True)
def _fresh_latch():
    rig._reset_for_tests()
    yield
    rig._reset_for_tests()


def _alive(tmp_path):
    """pids the stub ranks left in tmp_path that still name a process"""
    alive = []
    for f in tmp_path.glob("*.pid"):
        pid = int(f.read_text())
        try:
            os.kill(pid, 0)
            alive.append(pid)
        except ProcessLookupError:
            pass
    return alive


# ---- launcher -------------------------------------------------------------------------------------------------------------------------------------------------
def test_plain_ranks_come_back_in_rank_order(tmp_path):
    a, b = rig.run_ranks("rig_stub_worker.py", tmp_path, "plain", tag="stub", timeout=20)
    assert (a["rank"], b["rank"]) == (0, 1)
    for r, res in enumerate((a, b)):
        assert res["argv"][:2] == [str(r), "2"] and int(res["argv"][2]) > 0 and res["argv"][3:] == [str(tmp_path / f"stub{r}.json"), "plain"]
        assert res["ipc_legacy"] == "0"
    assert a["argv"][2] == b["argv"][2] and not rig.FAULTED and not _alive(tmp_path)


def test_an_ordinary_failure_fails_the_call_and_leaves_the_latch_alone(tmp_path):
    with pytest.raises(AssertionError):
        rig.run_ranks("rig_stub_worker.py", tmp_path, "exit3", timeout=20)
    assert not rig.FAULTED and not _alive(tmp_path)
    assert len(rig.run_ranks("rig_stub_worker.py", tmp_path, "plain", timeout=20)) == 2      # the next call runs


def test_a_fault_status_sets_the_latch_and_nothing_is_started_after_it(tmp_path):
    first, second = tmp_path / "first", tmp_path / "second"
    first.mkdir(); second.mkdir()
    t0 = time.monotonic()
    with pytest.raises(AssertionError):
        rig.run_ranks("rig_stub_worker.py", first, "exit139", timeout=20)      # rank 1 sleeps: it is killed, not waited for
    assert time.monotonic() - t0 < 10 and not _alive(first)
    assert len(rig.FAULTED) == 1 and "rank 0" in rig.FAULTED[0] and "139" in rig.FAULTED[0]
    with pytest.raises(pytest.fail.Exception, match="not run"):
        rig.run_ranks("rig_stub_worker.py", second, "plain", timeout=20)
    assert list(second.iterdir()) == []                                        # no rank ran: not even its pid file is there
    with pytest.raises(pytest.fail.Exception, match="not run"):
        rig.stop_after_fault()


def test_a_timeout_kills_both_ranks_and_sets_the_latch(tmp_path):
    import subprocess
    t0 = time.monotonic()
    with pytest.raises(subprocess.TimeoutExpired):
        rig.run_ranks("rig_stub_worker.py", tmp_path, "sleep", timeout=1)
    assert time.monotonic() - t0 < 10 and not _alive(tmp_path)
    assert len(rig.FAULTED) == 1 and "1 s" in rig.FAULTED[0]


def test_world_is_at_most_two(tmp_path):
    with pytest.raises(AssertionError):
        rig.run_ranks("rig_stub_worker.py", tmp_path, "plain", world=3, timeout=20)
    assert list(tmp_path.iterdir()) == []


def test_sync_records_a_runtime_error_and_raises_it_again(monkeypatch):
    def broken():
        raise RuntimeError("HIP error: an illegal memory access was encountered")
    monkeypatch.setattr(torch.cuda, "synchronize", broken)
    with pytest.raises(RuntimeError, match="illegal memory access"):
        rig.sync()
    assert rig.FAULTED == ["HIP error: an illegal memory access was encountered"]


# ---- step rig -------------------------------------------------------------------------------------------------------------------------------------------------
def test_seeded_models_are_a_function_of_the_seeds():
    cfg = rig.small_cfg(width_div=16)
    assert cfg.batchsize == 2 and cfg.width == {k: v // 16 for k, v in rig.small_cfg(width_div=1).width.items()}
    (m1, r1), (m2, r2), (m3, _) = (rig.seeded_models(cfg, CPU, s, 9) for s in (21, 21, 22))
    assert all(m._rng is r1 for m in m1.values()) and len(m1) == 5 and r1 is not r2
    a, b, c = (rig.state_bytes(m) for m in (m1, m2, m3))
    assert a.keys() == b.keys() == c.keys() and len(a) > 50
    assert all(torch.equal(a[k], b[k]) for k in a) and rig.sha_of(a.values()) == rig.sha_of(b.values())
    assert any(not torch.equal(a[k], c[k]) for k in a) and rig.sha_of(a.values()) != rig.sha_of(c.values())
    assert r1.state_dict() == dict(fixed_seed=9, seed_seen=None, counter=0)


def test_clip_pair_is_the_written_out_formula():
    cfg = rig.small_cfg()
    xc, xg = rig.clip_pair(cfg, CPU, 4, batch=1, frames=2, size=4)
    g = torch.Generator().manual_seed(4)
    want_c = torch.rand(1, 3, 2, 4, 4, generator=g) * 2 - 1
    want_g = torch.rand(1, cfg.channel, 2, 4, 4, generator=g) * 2 - 1
    assert torch.equal(xc, want_c) and torch.equal(xg, want_g)
    _, x1 = rig.clip_pair(cfg, CPU, 4, batch=1, frames=2, size=4, geo_channels=1)
    assert tuple(x1.shape) == (1, 1, 2, 4, 4) and torch.equal(x1, want_g[:, :1]) == (cfg.channel == 1)


class _Runner:
    """Notes the sync-debug mode every step runs under (`mode`: the list the patched torch.cuda.set_sync_debug_mode appends to)"""
    def __init__(self, mode, fail_at):
        self.mode, self.fail_at, self.modes = mode, fail_at, []

    def step(self, xc, xg, t):
        self.modes.append(self.mode[-1])
        if t == self.fail_at:
            raise ValueError("step failed")
        return {"t": t}


def test_counted_steps_arms_from_the_given_step_and_always_restores(monkeypatch):
    from dcvgan_amd import native
    mode = ["default"]
    monkeypatch.setattr(torch.cuda, "set_sync_debug_mode", mode.append)      # (the real one needs a device)
    n0 = native.launch_count()
    r = _Runner(mode, fail_at=None)
    counts, outs = rig.counted_steps(r, None, None, [3, 4, 5], strict_from=1)
    assert counts == [0, 0, 0] and outs == [{"t": 3}, {"t": 4}, {"t": 5}] and native.launch_count() == n0
    assert r.modes == ["default", "error", "error"] and mode == ["default", "error", "default"]
    del mode[1:]
    r = _Runner(mode, fail_at=4)
    with pytest.raises(ValueError):
        rig.counted_steps(r, None, None, [3, 4, 5])
    assert r.modes == ["error", "error"] and mode == ["default", "error", "default"]
