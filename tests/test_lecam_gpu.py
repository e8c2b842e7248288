"""GPU: dcv_lecam_sums / dcv_lecam_apply against their numpy restatement (tests/test_lecam_cpu.py) with exact equality, and the iteration with lecam.LeCam."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import rig
from tests import test_lecam_cpu as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F32, F64 = np.float32, np.float64
PAD = 8            # floats of sentinel on either side of every tensor the kernel writes
SENTINEL = 12345.5
SIZES = [(1, 1), (255, 257), (256, 256), (32, 128), (1123, 4099)]


def _padded(values):
    """-> (the whole buffer, the view the kernel gets): `values` between two runs of sentinels."""
    v = np.asarray(values, dtype=F32).reshape(-1)
    buf = torch.full((v.size + 2 * PAD,), SENTINEL, dtype=torch.float32, device=DEV)
    buf[PAD:PAD + v.size] = torch.from_numpy(v).to(DEV)
    return buf, buf[PAD:PAD + v.size]


def _intact(buf):
    return bool((buf[:PAD] == SENTINEL).all()) and bool((buf[-PAD:] == SENTINEL).all())


def _tab(ts, ctype=C.c_void_p):
    return (ctype * len(ts))(*[t.data_ptr() if isinstance(t, torch.Tensor) else int(t) for t in ts])


def _call(y_reals, y_fakes, state, decay, start, weight, one_sided, losses, dy_reals, dy_fakes):
    """One dcv_lecam_sums + dcv_lecam_apply on device tensors; -> (sums, reg) as numpy.  `state`, `losses`, `dy_*` are modified in place."""
    from dcvgan_amd import native
    L, s, n = native.lib(), native.stream_ptr(), len(y_reals)
    sums = torch.full((n, 4), float("nan"), dtype=torch.float64, device=DEV)
    reg = torch.full((n + 2,), SENTINEL, dtype=torch.float32, device=DEV)
    yr, yf = _tab(y_reals), _tab(y_fakes)
    nr, nf = _tab([t.numel() for t in y_reals], C.c_int64), _tab([t.numel() for t in y_fakes], C.c_int64)
    n0 = native.launch_count()
    native.check(L.dcv_lecam_sums(n, yr, yf, nr, nf, native.ptr(sums), s), "dcv_lecam_sums")
    native.check(L.dcv_lecam_apply(n, yr, yf, nr, nf, native.ptr(sums), native.ptr(state), float(decay), int(start), float(weight), int(one_sided),
                                   _tab(losses), _tab(dy_reals), _tab(dy_fakes), native.ptr(reg[1:]), s), "dcv_lecam_apply")
    assert native.launch_count() - n0 == 2
    torch.cuda.synchronize()
    reg = reg.cpu().numpy()
    assert reg[0] == SENTINEL and reg[-1] == SENTINEL
    return sums.cpu().numpy(), reg[1:-1]


def _bits(a):
    return np.asarray(a, dtype=F32).reshape(-1).view(np.uint32)


def _logits(gen, n, exact):
    if exact:
        return (gen.integers(-2047, 2048, size=n).astype(F64) / 256.0).astype(F32)      # multiples of 2^-8, |y| < 8
    return (gen.standard_normal(n) * 1.5 + 0.25).astype(F32)


def _sizes_of(n_dis, i):
    """Discriminator k of case i takes SIZES[(i + k) % 5]: a table of unequal tensors."""
    return [SIZES[(i + k) % len(SIZES)] for k in range(n_dis)]


# ---- 1. exact equality with the restatement -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(range(len(SIZES))) + ["exact"])
def test_exact_bit_for_bit(case):
    """Three consecutive calls from a zeroed state (the first update, the EMA, the start switch), n_dis 1 and 3, one- and two-sided, start 0 and 2; loss and dy
    pre-filled; every word of the state, loss, dy, reg and sums equals the restatement's; nothing is written outside the tensors."""
    exact = case == "exact"
    i = 4 if exact else case
    gen = np.random.default_rng(100 + i)
    checked = changed = 0
    for n_dis in (1, 3):
        sizes = _sizes_of(n_dis, i)
        for one_sided in (0, 1):
            for start in (0, 2):
                state_dev = torch.zeros(n_dis * 8, dtype=torch.int32, device=DEV)
                state = R.zero_state(n_dis)
                actives = []
                for call in range(3):
                    yr, yf = [_logits(gen, a, exact) for a, _ in sizes], [_logits(gen, b, exact) for _, b in sizes]
                    loss0 = [F32(v) for v in gen.standard_normal(n_dis)]
                    dr0, df0 = [gen.standard_normal(y.shape).astype(F32) for y in yr], [gen.standard_normal(y.shape).astype(F32) for y in yf]
                    t_yr, t_yf = [torch.from_numpy(y).to(DEV) for y in yr], [torch.from_numpy(y).to(DEV) for y in yf]
                    b_loss, b_dr, b_df = [_padded([v]) for v in loss0], [_padded(d) for d in dr0], [_padded(d) for d in df0]
                    sums, reg = _call(t_yr, t_yf, state_dev, 0.9, start, 0.3, one_sided, [v for _, v in b_loss], [v for _, v in b_dr], [v for _, v in b_df])
                    want_sums = R.sums_ref(yr, yf)
                    state, w_loss, w_dr, w_df, w_reg = R.apply_ref(yr, yf, want_sums, state, 0.9, start, 0.3, bool(one_sided), loss0, dr0, df0)
                    where = (case, n_dis, one_sided, start, call)
                    assert np.array_equal(sums.view(np.int64), want_sums.view(np.int64)), where
                    assert [[int(v) for v in row] for row in state_dev.view(n_dis, 8).cpu().tolist()] == state, where
                    assert np.array_equal(_bits(reg), _bits(w_reg)), where
                    for k in range(n_dis):
                        assert np.array_equal(_bits(b_loss[k][1].cpu().numpy()), _bits(w_loss[k])), where + (k,)
                        assert np.array_equal(_bits(b_dr[k][1].cpu().numpy()), _bits(w_dr[k])), where + (k,)
                        assert np.array_equal(_bits(b_df[k][1].cpu().numpy()), _bits(w_df[k])), where + (k,)
                        assert _intact(b_loss[k][0]) and _intact(b_dr[k][0]) and _intact(b_df[k][0]), where + (k,)
                        changed += int(state[k][R.ACTIVE] and not np.array_equal(_bits(w_dr[k]), _bits(dr0[k])) and w_reg[k] > 0)
                    actives.append([s[R.ACTIVE] for s in state])
                    checked += 1
                assert [s[R.UPDATES] for s in state] == [3] * n_dis
                assert actives == ([[0] * n_dis, [1] * n_dis, [1] * n_dis] if start == 0 else [[0] * n_dis, [0] * n_dis, [1] * n_dis])
    assert checked == 24 and changed >= 8      # the active calls did add something


# ---- 2. inactive ------------------------------------------------------------------------------------------------------------------------------------------------
def test_inactive_call_writes_no_byte():
    gen = np.random.default_rng(7)
    sizes = _sizes_of(3, 1)
    yr, yf = [_logits(gen, a, False) for a, _ in sizes], [_logits(gen, b, False) for _, b in sizes]
    dr0, df0 = [gen.standard_normal(y.shape).astype(F32) for y in yr], [gen.standard_normal(y.shape).astype(F32) for y in yf]
    dr0[0][0] = np.nan      # untouched means untouched: an inactive path that added 0 could not be told from this one on finite values alone
    loss0 = [F32(0.5), F32(-2.0), F32(np.nan)]
    state0 = [[R.f32_bits(0.5), R.f32_bits(-0.5), 4, 1, 0, 0, 0, 0] for _ in range(3)]
    state_dev = torch.tensor(state0, dtype=torch.int32).reshape(-1).to(DEV)
    b_loss, b_dr, b_df = [_padded([v]) for v in loss0], [_padded(d) for d in dr0], [_padded(d) for d in df0]
    before = [b.clone() for b, _ in b_loss + b_dr + b_df]
    t_yr, t_yf = [torch.from_numpy(y).to(DEV) for y in yr], [torch.from_numpy(y).to(DEV) for y in yf]
    _, reg = _call(t_yr, t_yf, state_dev, 0.99, 1000, 0.3, 1, [v for _, v in b_loss], [v for _, v in b_dr], [v for _, v in b_df])
    for (b, _), b0 in zip(b_loss + b_dr + b_df, before):
        assert torch.equal(b.view(torch.int32), b0.view(torch.int32))
    assert np.array_equal(_bits(reg), np.zeros(3, dtype=np.uint32))
    got = state_dev.view(3, 8).cpu().tolist()
    want, _, _, _, _ = R.apply_ref(yr, yf, R.sums_ref(yr, yf), state0, 0.99, 1000, 0.3, True, loss0, dr0, df0)
    assert got == want
    for k in range(3):
        assert got[k][R.ACTIVE] == 0 and got[k][R.UPDATES] == 5 and got[k][:2] != state0[k][:2]      # the anchors have moved


# ---- 3. a non-finite mean -------------------------------------------------------------------------------------------------------------------------------------
def test_non_finite_mean_freezes_that_discriminator_only():
    gen = np.random.default_rng(8)
    sizes = _sizes_of(3, 2)
    yr, yf = [_logits(gen, a, False) for a, _ in sizes], [_logits(gen, b, False) for _, b in sizes]
    yr[1][yr[1].size // 2] = np.nan
    state0 = [[R.f32_bits(0.25 * (k + 1)), R.f32_bits(-0.25 * (k + 1)), 2, 0, 0, 0, 0, 0] for k in range(3)]
    state_dev = torch.tensor(state0, dtype=torch.int32).reshape(-1).to(DEV)
    dr0, df0 = [np.zeros_like(y) for y in yr], [np.zeros_like(y) for y in yf]
    b_loss, b_dr, b_df = [_padded([0.0]) for _ in range(3)], [_padded(d) for d in dr0], [_padded(d) for d in df0]
    t_yr, t_yf = [torch.from_numpy(y).to(DEV) for y in yr], [torch.from_numpy(y).to(DEV) for y in yf]
    sums, _ = _call(t_yr, t_yf, state_dev, 0.9, 1000, 0.3, 1, [v for _, v in b_loss], [v for _, v in b_dr], [v for _, v in b_df])
    got = state_dev.view(3, 8).cpu().tolist()
    want, _, _, _, _ = R.apply_ref(yr, yf, R.sums_ref(yr, yf), state0, 0.9, 1000, 0.3, True, [F32(0)] * 3, dr0, df0)
    assert math.isnan(sums[1][0]) and np.isfinite(sums[[0, 2]]).all()
    assert got == want and got[1] == state0[1]
    for k in (0, 2):
        assert got[k][R.UPDATES] == 3 and got[k][:2] != state0[k][:2]


# ---- 4. - 6. the iteration ------------------------------------------------------------------------------------------------------------------------------------
def _runner(lecam_kw, seed=21, pass_arg=True, sync_losses=False):
    from dcvgan_amd import native, trainer
    native.lib()
    cfg = rig.small_cfg()
    models, _ = rig.seeded_models(cfg, DEV, seed, 9)
    opts = trainer.build_optimizers(cfg, models)
    lc = trainer.build_lecam(cfg, models, opts, **lecam_kw) if lecam_kw is not None else None
    kw = dict(lecam=lc) if pass_arg else {}
    return cfg, models, opts, lc, trainer.StepRunner(cfg, models, opts, trainer.build_loss(cfg), sync_losses=sync_losses, **kw)


def _data(cfg):
    return rig.clip_pair(cfg, DEV, 4)


_counted_steps = rig.counted_steps
_snapshot = rig.state_bytes      # every parameter, buffer and Adam moment, as bytes


def _loss_bits(out):
    return {k: R.f32_bits(float(v)) for k, v in out.items() if k.startswith("loss_")}


def test_iteration():
    """The regulariser on (two-sided here: with a handful of logits per discriminator a one-sided term can be exactly 0, and this test asks for > 0): no torch
    kernel, no host sync, two launches more than the plain iteration, finite outputs, active from the second iteration with start = 0."""
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    cfg, models, opts, lc, runner = _runner(dict(weight=0.3, start=0, one_sided=False))
    xc, xg = _data(cfg)
    runner.step(xc, xg, 2)      # warm-up: optimiser state, workspaces and pointer tables are made here; the anchors' first update
    torch.cuda.synchronize()
    assert [w[R.UPDATES] for w in lc.state_words()] == [1, 1, 1] and [w[R.ACTIVE] for w in lc.state_words()] == [0, 0, 0]
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        (c2, c3), (o2, o3) = _counted_steps(runner, xc, xg, [3, 4])
        torch.cuda.synchronize()
    kernels = {e.key: e.count for e in prof.key_averages() if e.device_type == DeviceType.CUDA}
    foreign = {k[:160]: n for k, n in kernels.items() if "at::" in k or "torch" in k.lower()}
    assert not foreign, foreign
    mine = {k[:60]: n for k, n in kernels.items() if "lecam" in k}
    assert sorted(mine.values()) == [2, 2] and any("lecam_sums" in k for k in mine) and any("lecam_apply" in k for k in mine), mine
    for o in (o2, o3):
        assert all(math.isfinite(float(v)) for v in o.values()), o
        assert all(float(o[k]) > 0 for k in ("lecam_idis", "lecam_vdis", "lecam_gdis")), o
    assert [w[R.UPDATES] for w in lc.state_words()] == [3, 3, 3] and [w[R.ACTIVE] for w in lc.state_words()] == [1, 1, 1]
    assert torch.equal(lc.reg, torch.stack([o3["lecam_idis"], o3["lecam_vdis"], o3["lecam_gdis"]])) and not lc.reg.requires_grad
    assert tuple(lc.anchors().shape) == (3, 8) and lc.anchors().is_cuda and all(math.isfinite(a) and math.isfinite(b) for a, b in lc.anchor_values())
    # launches: the plain run plus 2
    cfg_p, _, _, _, plain = _runner(None)
    plain.step(xc, xg, 2)
    (p2, p3), _ = _counted_steps(plain, xc, xg, [3, 4])
    print(f"\n[lecam iteration] launches per iteration {c2}, {c3} vs plain {p2}, {p3}; kernels {mine}; reg {[float(v) for v in lc.reg]}, anchors {lc.anchor_values()}")
    assert c2 == p2 + 2 and c3 == p3 + 2
    # lecam=None, and a StepRunner that was never given the argument: the same count
    _, _, _, _, bare = _runner(None, pass_arg=False)
    bare.step(xc, xg, 2)
    (b2, b3), _ = _counted_steps(bare, xc, xg, [3, 4])
    assert (b2, b3) == (p2, p3)
    # sync_losses: floats
    _, _, _, lc_s, synced = _runner(dict(weight=0.3, start=0, one_sided=False), sync_losses=True)
    synced.step(xc, xg, 2)
    o = synced.step(xc, xg, 3)
    assert all(isinstance(o[k], float) and o[k] > 0 for k in ("lecam_idis", "lecam_vdis", "lecam_gdis")), o
    assert _loss_bits(o) == _loss_bits(o2)      # the same run, read the reference's way


def test_inactive_iterations_are_bit_identical_to_the_plain_run():
    """start beyond the run, three iterations: every parameter, buffer, Adam moment and loss is the plain run's, bit for bit."""
    runs = {}
    for name, kw in (("plain", None), ("lecam", dict(weight=0.3, start=1000))):
        cfg, models, opts, lc, runner = _runner(kw)
        xc, xg = _data(cfg)
        outs = [runner.step(xc, xg, 2 + it) for it in range(3)]
        runs[name] = dict(snap=_snapshot(models, opts), losses=[_loss_bits(o) for o in outs], lc=lc, outs=outs)
    a, b = runs["plain"], runs["lecam"]
    assert a["losses"] == b["losses"] and len(a["losses"][0]) == 4
    assert a["snap"].keys() == b["snap"].keys() and len(a["snap"]) > 100
    assert all(torch.equal(a["snap"][k], b["snap"][k]) for k in a["snap"])
    assert all(float(o[k]) == 0.0 for o in b["outs"] for k in ("lecam_idis", "lecam_vdis", "lecam_gdis"))
    words = b["lc"].state_words()
    assert [w[R.UPDATES] for w in words] == [3, 3, 3] and [w[R.ACTIVE] for w in words] == [0, 0, 0] and all(w[0] != 0 and w[1] != 0 for w in words)


def test_state_dict_round_trip():
    """Two runs from the same seeds, two iterations each (active from the second); then one of them goes on with a FRESH LeCam loaded from the other's
    state_dict: the next iteration's losses and regulariser terms are bit-identical.  A fresh one that was not loaded gives other losses."""
    from dcvgan_amd import trainer
    kw = dict(weight=0.3, start=0)
    third = {}
    for name in ("kept", "loaded", "fresh"):
        cfg, models, opts, lc, runner = _runner(kw)
        xc, xg = _data(cfg)
        for it in range(2):
            runner.step(xc, xg, 2 + it)
        if name != "kept":
            sd = lc.state_dict()
            assert [w[R.UPDATES] for w in sd["state"]] == [2, 2, 2]
            new = trainer.build_lecam(cfg, models, opts, weight=0.1, start=5, decay=0.5)
            if name == "loaded":
                new.load_state_dict(sd)
                assert new.state_words() == sd["state"] and (new.weight, new.start, new.decay) == (0.3, 0, 0.99)
            else:
                new.weight, new.start, new.decay = 0.3, 0, 0.99
            runner.lecam = new
        o = runner.step(xc, xg, 4)
        torch.cuda.synchronize()
        third[name] = {k: R.f32_bits(float(v)) for k, v in o.items()}
    print(f"\n[lecam state_dict] third iteration {third['kept']}")
    assert third["kept"] == third["loaded"]
    assert third["fresh"] != third["kept"] and all(third["fresh"][k] == 0 for k in ("lecam_idis", "lecam_vdis", "lecam_gdis"))
    assert any(third["kept"][k] != 0 for k in ("lecam_idis", "lecam_vdis", "lecam_gdis"))
