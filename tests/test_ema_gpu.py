"""GPU: the device-side EMA of the generators' weights — dcv_ema_update_multi against an fp64 evaluation of e + (1 - d_t)(p - e) on the host,
the warm-up schedule and the device count, copy mode, the guard's skip, no host wait and no torch kernel, repeatability, the packed-weight caches of the twin,
the update inside trainer.StepRunner, and the checkpoint round trip.  Every case prints its figures (pytest -s).

The bar everywhere: |e - e64| <= k * 2^-21 * M after k updates, M the largest magnitude among the inputs.  One update rounds 1 - d, p - e and the fma once each;
|p - e| <= 2M and |e'| <= M, so it adds at most 5 * 2^-24 M, and earlier error is carried with the factor 1 - w <= 1; 2^-21 = 8 * 2^-24 leaves the rest as margin."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import rig

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BAR = 2.0 ** -21


def _decay(t, decay=0.999, warmup=True):
    return min(decay, (1.0 + t) / (10.0 + t)) if warmup else decay


def _update(es, ss, modes, decay, warmup, block, state=None):
    from dcvgan_amd.native import c_array as arr, check, lib, ptr, stream_ptr
    dwords = arr([e.numel() * (e.element_size() // 4) for e in es], C.c_int64)
    check(lib().dcv_ema_update_multi(len(es), arr(es), arr(ss), dwords, arr(modes, C.c_int32), decay, int(warmup), ptr(block), ptr(state), stream_ptr()), "dcv_ema_update_multi")


def _block():
    return torch.zeros(16, dtype=torch.int32).to(DEV)


GUARD = 8      # elements of NaN on either side of every tensor (a 32-byte band: the view behind it stays 16-byte aligned)


def _banded(n, off, gen, scale):
    """A length-n fp32 view at element offset GUARD + off of a NaN-filled buffer; off = 1 leaves it only 4-byte aligned."""
    buf = torch.full((n + 2 * GUARD + 4,), float("nan"), dtype=torch.float32)
    buf[GUARD + off:GUARD + off + n] = torch.randn(n, generator=gen) * scale
    buf = buf.to(DEV)
    return buf, buf[GUARD + off:GUARD + off + n]


def _bands_intact(buf, view):
    if view.numel() == 0:
        return bool(torch.isnan(buf).all())
    a = (view.data_ptr() - buf.data_ptr()) // 4
    return bool(torch.isnan(buf[:a]).all() and torch.isnan(buf[a + view.numel():]).all())


def _kernel_case():
    g = torch.Generator().manual_seed(11)
    sizes = [0, 1, 2, 3, 4, 5, 255, 256, 257, 4095, 4096, 4097, 8193, 3 * 4096 + 2]
    sizes += [int(v) for v in torch.randint(1, 20000, (30 - len(sizes),), generator=g)]
    # tensor index -> (ema offset, source offset): three views at element offset 1 on both sides, one with only the source off the 16-byte grid
    offs = {5: (1, 1), 11: (1, 1), 20: (1, 1), 12: (0, 1)}
    modes = [0] * 30
    modes[7], modes[27] = 1, 1      # a copied tensor in each of the two launches
    modes[20] = 1                   # and one off the 16-byte grid on both sides: the copy's per-element path
    ebufs, es = zip(*[_banded(n, offs.get(i, (0, 0))[0], g, 3.0) for i, n in enumerate(sizes)])
    return sizes, offs, modes, g, ebufs, es


def test_kernel_against_fp64():
    from dcvgan_amd import native
    native.lib()
    k = 5
    sizes, offs, modes, g, ebufs, es = _kernel_case()
    assert sum(1 for e in es if e.data_ptr() % 16) == 3 and all(e.data_ptr() % 4 == 0 for e in es) and all(e.data_ptr() for e in es[1:])
    e64 = [e.cpu().double() for e in es]
    big = max([float(e.abs().max()) for e in es if e.numel()])
    block = _block()
    for t in range(k):
        sbufs, ss = zip(*[_banded(n, offs.get(i, (0, 0))[1], g, 2.0 + t) for i, n in enumerate(sizes)])      # the sources change between updates
        assert ss[12].data_ptr() % 16 and es[12].data_ptr() % 16 == 0
        big = max([big] + [float(s.abs().max()) for s in ss if s.numel()])
        n0 = native.launch_count()
        _update(es, ss, modes, 0.999, True, block)
        assert native.launch_count() - n0 == 1 + math.ceil(30 / 24)
        w = 1.0 - _decay(t)
        for i in range(30):
            e64[i] = ss[i].cpu().double() if modes[i] else e64[i] + w * (ss[i].cpu().double() - e64[i])
        torch.cuda.synchronize()
        assert all(_bands_intact(b, v) for b, v in zip(sbufs, ss))
        assert all(torch.equal(es[i].view(torch.int32), ss[i].view(torch.int32)) for i in (7, 20, 27))      # copy mode: bit for bit
    assert all(_bands_intact(b, v) for b, v in zip(ebufs, es)), "an EMA tensor's NaN guard band was written"
    worst = 0.0
    for i in range(30):
        if sizes[i]:
            err = float((es[i].cpu().double() - e64[i]).abs().max())
            worst = max(worst, err / (k * BAR * big))
            assert err <= k * BAR * big, (i, sizes[i], err, k * BAR * big)
    assert int(block[0]) == k
    print(f"\n[ema kernel] 30 tensors, {k} updates, M = {big:.3f}: worst error / bar = {worst:.3f}")


def test_warmup_schedule_and_count():
    from dcvgan_amd import native
    native.lib()
    e, p = torch.zeros(1).to(DEV), torch.ones(1).to(DEV)
    block = _block()
    got = []
    for t in range(12):
        _update([e], [p], [0], 0.999, True, block)
        got.append(e.clone())
    got = [float(v) for v in got]
    want, x = [], 0.0
    for t in range(12):
        x = x + (1.0 - _decay(t)) * (1.0 - x)
        want.append(x)
    worst = max(abs(a - b) / ((t + 1) * BAR) for t, (a, b) in enumerate(zip(got, want)))
    print(f"\n[ema warm-up] e after 12 updates {got[-1]:.9f} (fp64 {want[-1]:.9f}); worst error / bar = {worst:.3f}")
    assert all(abs(a - b) <= (t + 1) * BAR for t, (a, b) in enumerate(zip(got, want))), (got, want)
    assert abs(got[0] - 0.9) <= BAR and int(block[0]) == 12      # d_0 = 1 / 10, not the decay
    # without warm-up the decay holds from the first update
    e2, b2 = torch.zeros(1).to(DEV), _block()
    _update([e2], [p], [0], 0.999, False, b2)
    assert abs(float(e2) - 0.001) <= BAR and int(b2[0]) == 1, float(e2)
    assert float(e2) == float(torch.tensor(1.0 - 0.999, dtype=torch.float64).float())      # w itself: (float)(1 - d), times 1, plus 0


def test_copy_mode_is_bit_exact():
    from dcvgan_amd import native
    native.lib()
    special = torch.tensor([0x7fc00001, 0xffc12345 - (1 << 32), 0x80000000 - (1 << 32), 0x00000001, 0x7f800000, 0x3f800000, 0x7f7fffff], dtype=torch.int32)
    src_f = special.view(torch.float32).to(DEV)                     # NaNs with payloads, -0, a denormal, inf: arithmetic would not keep them
    dst_f = torch.randn(7).to(DEV)
    src_i = torch.tensor([2 ** 33 + 5, -7, 2 ** 62 + 3], dtype=torch.int64).to(DEV)
    dst_i = torch.zeros(3, dtype=torch.int64).to(DEV)
    # decay 0 -> w = 1: fmaf(1, p - e, e) with e = 1e8, p = 1 gives 0 (p - e rounds to -1e8); the copied twin of the same pair must hold 1
    e_avg, e_cpy = torch.full((6,), 1e8).to(DEV), torch.full((6,), 1e8).to(DEV)
    p = torch.ones(6).to(DEV)
    block = _block()
    _update([dst_f, dst_i, e_avg, e_cpy], [src_f, src_i, p, p], [1, 1, 0, 1], 0.0, False, block)
    torch.cuda.synchronize()
    assert torch.equal(dst_f.view(torch.int32).cpu(), special)
    assert torch.equal(dst_i.cpu(), src_i.cpu()) and int(dst_i[0]) == 2 ** 33 + 5      # both dwords arrived
    assert torch.equal(e_cpy, p) and float(e_avg[0]) == 0.0, (e_cpy, e_avg)
    print(f"\n[ema copy] int64 {int(dst_i[0])}; averaged (w = 1) {float(e_avg[0])} vs copied {float(e_cpy[0])}")


def _models(name="isogd-depth", width_div=8, seed=3, **kw):
    from dcvgan_amd import native, trainer
    native.lib()
    cfg = rig.small_cfg(name, width_div=width_div, **kw)
    torch.manual_seed(seed)
    return cfg, trainer.build_models(cfg, DEV)


def _bits(ema):
    return [v.clone() for n in ema.names for v in ema.module(n).state_dict().values()]


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x.reshape(-1).view(torch.uint8), y.reshape(-1).view(torch.uint8)) for x, y in zip(a, b))


def _move_live(models, step=0.125):
    with torch.no_grad():
        for n in ("ggen", "cgen"):
            for p in models[n].parameters():
                p.add_(step)


def test_guard_skip():
    from dcvgan_amd import optim, trainer
    cfg, models = _models()
    opts = trainer.build_optimizers(cfg, models, guard={})
    guard = opts["ggen"].guard
    ema, free = trainer.build_ema(cfg, models, opts, decay=0.9, warmup=False), optim.ModelEma(models, decay=0.9, warmup=False)
    assert ema.guard is guard and free.guard is None
    _move_live(models)
    params = [p for n in ("ggen", "cgen") for p in models[n].parameters()]
    for p in params:
        p.grad = torch.full_like(p, 1e-3)
    params[3].grad.view(-1)[0] = float("inf")
    guard.measure()
    before, before_free = _bits(ema), _bits(free)
    ema.update(); free.update()
    torch.cuda.synchronize()
    assert float(guard.stats()["skipped"]) == 1.0
    assert _same(_bits(ema), before) and ema.num_updates() == 0, "a skipped update wrote a twin or advanced the count"
    assert not _same(_bits(free), before_free) and free.num_updates() == 1      # without a guard it always advances
    params[3].grad.view(-1)[0] = 1e-3
    guard.measure()
    ema.update(); free.update()
    torch.cuda.synchronize()
    assert float(guard.stats()["skipped"]) == 0.0
    assert not _same(_bits(ema), before) and ema.num_updates() == 1 and free.num_updates() == 2
    # the applied update is the first one: e + 0.1 (p - e) with p - e = 0.125
    e, p = ema.module("cgen").outconv.main[0].weight, models["cgen"].outconv.main[0].weight
    err = float((e.double() + 0.9 * 0.125 - p.double()).abs().max())
    print(f"\n[ema guard] skipped, then applied: count {ema.num_updates()}, |e - e64| max {err:.2e}")
    assert err <= BAR * float(p.abs().max())


def test_update_waits_for_nothing_and_counts_its_launches():
    from dcvgan_amd import native, optim
    cfg, models = _models()
    ema = optim.ModelEma(models)
    ema.update()      # builds the pointer tables
    tables = dict(ema._tables)
    n0 = native.launch_count()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ema.update()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    want = sum(1 + math.ceil(sum(1 for v in models[n].state_dict().values() if v.numel()) / 24) for n in ("ggen", "cgen"))
    got = native.launch_count() - n0
    print(f"\n[ema launches] {got} per update ({', '.join('%s: %d tensors' % (n, len(models[n].state_dict())) for n in ('ggen', 'cgen'))})")
    assert got == want
    assert all(ema._tables[n] is tables[n] for n in tables), "the pointer tables were rebuilt although no data_ptr changed"
    assert ema.num_updates() == 2


@pytest.mark.parametrize("config,cl", [("isogd-depth", False), ("surreal-depth1", True)], ids=["isogd-depth", "surreal-depth1-bf16cl"])
def test_no_torch_compute_kernel_in_the_iteration_with_ema(config, cl):
    """tests/test_grad_accumulation_gpu.py::test_no_torch_compute_kernel_in_the_iteration with ema=: the same filter."""
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    from dcvgan_amd import ops_cl, trainer
    from dcvgan_amd.configs import CONFIGS
    from dcvgan_amd.rng import PhiloxRng
    cfg = CONFIGS[config].scaled(batchsize=2, width_div=4)
    torch.manual_seed(1)
    ops_cl.enable(cl)
    try:
        models = trainer.build_models(cfg, DEV)
        r = PhiloxRng(5)
        for m in models.values():
            m._rng = r
        xc = torch.rand(2, 3, 16, 64, 64, device=DEV) * 2 - 1; xg = torch.rand(2, cfg.channel, 16, 64, 64, device=DEV) * 2 - 1
        opts = trainer.build_optimizers(cfg, models)
        ema = trainer.build_ema(cfg, models, opts)
        runner = trainer.StepRunner(cfg, models, opts, trainer.build_loss(cfg), sync_losses=False, ema=ema)
        for t in (1, 2):
            runner.step(xc, xg, t)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            runner.step(xc, xg, 3)
            runner.step(xc, xg, 4)
            torch.cuda.synchronize()
    finally:
        ops_cl.enable(False)
    kernels = {e.key: e.count for e in prof.key_averages() if e.device_type == DeviceType.CUDA}
    foreign = {k[:160]: n for k, n in kernels.items() if "at::" in k or "torch" in k.lower()}
    assert not foreign, foreign
    mine = {k[:60]: n for k, n in kernels.items() if "ema_" in k}
    print(f"\n[ema in the iteration, {config}{' bf16cl' if cl else ''}] {mine}")
    assert any("ema_prepare" in k for k in kernels) and any("ema_multi" in k for k in kernels), sorted(kernels)[:40]
    assert ema.num_updates() == 4


def test_repeatable():
    from dcvgan_amd import native
    native.lib()
    runs = []
    for _ in range(2):
        sizes, offs, modes, g, ebufs, es = _kernel_case()
        block = _block()
        for t in range(3):
            sbufs, ss = zip(*[_banded(n, offs.get(i, (0, 0))[1], g, 2.0) for i, n in enumerate(sizes)])
            _update(es, ss, modes, 0.99, True, block)
        torch.cuda.synchronize()
        runs.append([e.clone() for e in es])
    assert _same(runs[0], runs[1])


@pytest.mark.parametrize("cl", [False, True], ids=["fp32", "bf16cl"])
def test_packed_weights_follow_the_twin(cl):
    """The twin's packed weights are cached by autograd version: update() writes through raw pointers and has to bump it."""
    from dcvgan_amd import ops_cl, optim, trainer
    from dcvgan_amd.rng import InjectedRng
    cfg, models = _models()
    g = torch.Generator().manual_seed(5)
    xs = (torch.rand(2, cfg.channel, 16, 64, 64, generator=g) * 2 - 1).to(DEV)
    log = [("normal", torch.randn(2, cfg.dim_z_color, generator=g))]

    def forward(m):
        m._rng = InjectedRng(log)
        with torch.no_grad():
            return m.forward_videos(xs).clone()
    ops_cl.enable(cl)
    try:
        ema = optim.ModelEma(models, decay=0.5, warmup=False)
        twin = ema.module("cgen")
        y0 = forward(twin)      # packs are cached now
        _move_live(models, 0.03125)
        ema.update()
        y1 = forward(twin)
        fresh = trainer.build_models(cfg, DEV)["cgen"]
        fresh.load_state_dict(twin.state_dict())
        y2 = forward(fresh.eval())
    finally:
        ops_cl.enable(False)
    torch.cuda.synchronize()
    print(f"\n[ema packs, {'bf16cl' if cl else 'fp32'}] forward moved by {float((y1 - y0).abs().max()):.3e}; twin vs fresh model {float((y1 - y2).abs().max()):.3e}")
    assert not torch.equal(y0, y1), "the update did not reach the twin's forward"
    assert torch.equal(y1, y2), "the twin sampled from stale packed weights"


def _iterate(cfg_name, width_div, iters, with_ema, seed=21, **kw):
    from dcvgan_amd import trainer
    cfg, models = _models(cfg_name, width_div, seed, **kw)
    rig.share_rng(models, 9)
    xc, xg = rig.clip_pair(cfg, DEV, 4)
    opts = trainer.build_optimizers(cfg, models)
    ema = trainer.build_ema(cfg, models, opts) if with_ema else None
    start = {n: {k: v.detach().clone() for k, v in models[n].named_parameters()} for n in ("ggen", "cgen")}
    runner = trainer.StepRunner(cfg, models, opts, trainer.build_loss(cfg), sync_losses=True, ema=ema)
    losses, snaps, counts = [], [], []
    for it in range(iters):
        losses.append(runner.step(xc, xg, 2 + it))
        snaps.append({n: {k: v.detach().clone() for k, v in models[n].named_parameters()} for n in ("ggen", "cgen")})
        counts.append(ema.num_updates() if ema is not None else None)
    return dict(cfg=cfg, models=models, opts=opts, ema=ema, start=start, losses=losses, snaps=snaps, counts=counts)


@pytest.fixture(scope="module")
def run():
    return _iterate("isogd-depth", 4, 3, True)


def test_in_the_iteration(run):
    ema, models, k = run["ema"], run["models"], 3
    assert run["counts"] == [1, 2, 3]
    worst = 0.0
    for n in ("ggen", "cgen"):
        twin = dict(ema.module(n).named_parameters())
        for key, e0 in run["start"][n].items():
            e64, big = e0.double(), float(e0.abs().max())
            for t in range(k):
                p = run["snaps"][t][n][key].double()
                big = max(big, float(p.abs().max()))
                e64 = e64 + (1.0 - _decay(t)) * (p - e64)
            err = float((twin[key].double() - e64).abs().max())
            worst = max(worst, err / (k * BAR * big))
            assert err <= k * BAR * big, (n, key, err, k * BAR * big)
        live_b, twin_b = dict(models[n].named_buffers()), dict(ema.module(n).named_buffers())
        assert list(live_b) == list(twin_b) and len(live_b) > 0
        assert _same([twin_b[b] for b in live_b], [live_b[b] for b in live_b]), n
        assert int(twin_b[next(b for b in twin_b if b.endswith("num_batches_tracked"))]) > 0
    print(f"\n[ema in the iteration] 3 iterations, twins vs fp64 EMA of the snapshots: worst error / bar = {worst:.3f}")
    # the same seeded run without the EMA: the live models and the losses do not change by a bit
    plain = _iterate("isogd-depth", 4, 3, False)
    assert plain["losses"] == run["losses"], (plain["losses"], run["losses"])
    for n in ("ggen", "cgen"):
        assert all(torch.equal(plain["snaps"][-1][n][key], v) for key, v in run["snaps"][-1][n].items()), n
    for n in ("idis", "vdis", "gdis"):
        assert all(torch.equal(a, b) for a, b in zip(plain["models"][n].state_dict().values(), models[n].state_dict().values())), n


def test_twins_share_no_storage(run):
    ema, models, opts = run["ema"], run["models"], run["opts"]
    mine = {t.data_ptr() for n in ema.names for t in ema.module(n).state_dict().values()}
    theirs = set()
    for n in ema.names:
        theirs |= {t.data_ptr() for t in models[n].state_dict().values()}
        theirs |= {p.grad.data_ptr() for p in models[n].parameters() if p.grad is not None}
        theirs |= {s[k].data_ptr() for s in opts[n].state.values() for k in ("exp_avg", "exp_avg_sq")}
    assert len(theirs) > 3 * len(mine) // 2 and not mine & theirs
    for n in ema.names:
        twin = ema.module(n)
        assert type(twin) is type(models[n]) and not twin.training and not any(p.requires_grad or p.grad is not None for p in twin.parameters())
        assert twin._rng is not None and twin._rng is not models[n]._rng
        assert not any(k.startswith("_dcv_bucket") or k.startswith("_dcv_grad") for p in twin.parameters() for k in p.__dict__)


def test_twins_draw_from_one_stream():
    """One sampling batch draws the geometry twin's content latent and the colour twin's hidden latent.  A PhiloxRng is (seed, counter), so a stream per twin would
    give both the same values, flat index by flat index; on the ModelEma's one stream the draws are independent: no leading value repeats, before and after a reseed."""
    _, models = _models()
    from dcvgan_amd import optim
    ema = optim.ModelEma(models)
    ggen, cgen = ema.module("ggen"), ema.module("cgen")
    assert ggen._rng is cgen._rng is ema.rng and all(ema.rng is not m.__dict__.get("_rng") for m in models.values())
    from dcvgan_amd.rng import default_rng
    assert ema.rng is not default_rng()
    for seed in (None, 1234):
        if seed is not None:
            torch.manual_seed(seed)
        B = 64
        zc = ggen.sample_z_content(B).view(B, ggen.video_length, ggen.dim_z_content)[:, 0].flatten().cpu()      # the draw itself, before the tiling over frames
        zh = cgen.make_hidden(B).flatten().cpu()
        k = min(zc.numel(), zh.numel())
        assert k >= 640
        same = int((zc[:k] == zh[:k]).sum())
        r = float(torch.corrcoef(torch.stack([zc[:k], zh[:k]]))[0, 1])
        print(f"\n[ema rng] seed {seed}: {same} of the first {k} values equal, correlation {r:+.3f}")
        # k independent N(0, 1) pairs: |r| < 5 / sqrt(k) fails once in ~2e6 draws, and these are fixed by the seed; equal streams give r = 1
        assert same == 0 and abs(r) < 5.0 / math.sqrt(k)


@pytest.mark.parametrize("gate,iters,want", [(1, 2, [1, 2]), (2, 3, [0, 1, 1])], ids=["preset", "num_dis_update=2"])
def test_count_follows_the_update_gating(gate, iters, want):
    """surreal-depth1 (num_gen_update = 2: the D phase steps every second iteration, the G phase every iteration), and the same with num_dis_update = 2, where the G
    phase of iterations 1 and 3 is gated off: the count advances only in iterations whose G phase stepped."""
    res = _iterate("surreal-depth1", 4, iters, True, num_dis_update=gate)
    assert res["cfg"].num_gen_update == 2
    print(f"\n[ema gating] num_dis_update = {gate}: counts {res['counts']}")
    assert res["counts"] == want == [sum(1 for i in range(1, it + 2) if i % gate == 0) for it in range(iters)]


def test_state_dict_round_trip_and_sampling(run):
    from dcvgan_amd import optim, sampling
    ema, models = run["ema"], run["models"]
    sd = ema.state_dict()
    assert list(sd) == ["ggen", "cgen", "num_updates", "decay", "warmup"] and sd["num_updates"] == 3
    assert all(list(sd[n]) == list(models[n].state_dict()) for n in ema.names)
    _, other_models = _models("isogd-depth", 4, seed=77)
    other = optim.ModelEma(other_models, decay=0.5, warmup=False)
    assert not _same(_bits(other), _bits(ema))
    other.load_state_dict({k: ({a: b.cpu() for a, b in v.items()} if isinstance(v, dict) else v) for k, v in sd.items()})      # as read back from a file
    assert _same(_bits(other), _bits(ema)) and other.num_updates() == 3 and other.decay == ema.decay and other.warmup == ema.warmup
    other.update()
    assert other.num_updates() == 4
    other.reset()
    assert other.num_updates() == 0 and _same(_bits(other), [v for n in other.names for v in other_models[n].state_dict().values()])
    xg, xc = sampling.generate_samples(ema.module("ggen"), ema.module("cgen"), num=2, batchsize=2)
    lg, lc = sampling.generate_samples(models["ggen"], models["cgen"], num=2, batchsize=2)
    assert xg.dtype == np.uint8 and xc.dtype == np.uint8
    assert xg.shape == lg.shape and xc.shape == lc.shape == (2, 3, 16, 64, 64)
    assert xc.std() > 0      # (uint8 is finite by construction: the clip is not one flat colour, as NaN activations would give)
    print(f"\n[ema sampling] twin clips {xc.shape}, mean byte {xc.mean():.1f}, std {xc.std():.1f}")
