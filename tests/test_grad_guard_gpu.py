"""GPU: optim.GradGuard — the device-side global gradient norm, clipping, non-finite skip and loss scale — and the guarded Adam step.

Where the bars come from:
  * norm, 1e-6 relative against fp64 on the host: a thread adds at most 16 squares in fp32, everything above that is double (a CPU emulation of this summation
    gave 4.4e-8);
  * clipped update, 2e-6 relative: the 1e-6 of tests/test_adam_gpu.py plus the coefficient's share (1.4e-7 in a CPU emulation).  The reference is torch.optim.Adam
    in fp32 on the host, fed gradients multiplied by a clip coefficient computed in fp64 on the host (torch's own fp32 clip_grad_norm_ is 3e-6 off the true norm at
    these sizes, so it is not the yardstick);
  * skip and loss-scale invariance: exact (torch.equal)."""
import copy
import math

import pytest
import torch

from tests import rig
from tests.test_adam_gpu import SIZES

pytestmark = pytest.mark.gpu
HP = dict(lr=2e-4, betas=(0.5, 0.999), eps=1e-8, weight_decay=1e-5)      # the reference's wiring
LATE = 4      # this tensor gets its first gradient at step 3
NORM_BAR, UPDATE_BAR = 1e-6, 2e-6


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _banded(g, dev, misaligned=False):
    """g as a view inside a larger NaN-filled device buffer: 64 floats of guard band on either side (the view starts 256 bytes, or 260 with `misaligned`, into it)."""
    off = 65 if misaligned else 64
    buf = torch.full((g.numel() + 130,), float("nan"), device=dev)
    view = buf[off:off + g.numel()].view(g.shape)
    view.copy_(g)
    assert view.data_ptr() % 16 == (4 if misaligned else 0)
    return view


def _draw(shape, gen):
    """magnitudes from 1e-6 to 1, as tests/test_adam_gpu.py draws them"""
    return torch.randn(shape, generator=gen) * (10.0 ** float(torch.randint(-6, 1, (1,), generator=gen)))


def _norm64(gs):
    return math.sqrt(sum(float((g.double() ** 2).sum()) for g in gs))


def _pair(gen, dev, guard):
    from dcvgan_amd import optim
    ref = [torch.nn.Parameter(torch.randn(s, generator=gen) * 0.05) for s in SIZES]
    hip = [torch.nn.Parameter(p.detach().clone().to(dev)) for p in ref]
    return ref, hip, torch.optim.Adam(ref, **HP), optim.Adam(hip, guard=guard, **HP)


def _compare(topt, hopt, ref, hip, bar, where):
    torch.cuda.synchronize()
    for i, (p, q) in enumerate(zip(ref, hip)):
        if p not in topt.state:
            assert q not in hopt.state and torch.equal(p.detach(), q.detach().cpu()), (where, i)
            continue
        st, sh = topt.state[p], hopt.state[q]
        assert int(st["step"]) == int(sh["step"].item()), (where, i, "step")
        assert _rel(q.detach(), p.detach()) <= bar, (where, i, "p")
        assert _rel(sh["exp_avg"], st["exp_avg"]) <= bar, (where, i, "m")
        assert _rel(sh["exp_avg_sq"], st["exp_avg_sq"]) <= bar, (where, i, "v")


def test_norm_against_fp64():
    from dcvgan_amd import optim
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(11)
    assert len(SIZES) == 30
    hip = [torch.nn.Parameter(torch.zeros(s, device=dev)) for s in SIZES]
    guard = optim.GradGuard()
    optim.Adam(hip, guard=guard, **HP)
    host = [_draw(s, gen) for s in SIZES]
    for i, (q, g) in enumerate(zip(hip, host)):
        q.grad = _banded(g, dev, misaligned=(i in (6, 16, 26)))      # (4095,), (512, 50, 4, 4) and (31, 31) start 4 bytes past a 16-byte boundary
    guard.measure()
    first = guard.state.clone()
    guard.measure()
    second = guard.state.clone()
    torch.cuda.synchronize()
    st = guard.stats()
    want = _norm64(host)
    got = float(st["grad_norm"])
    print("grad_norm %.9g, fp64 %.9g, relative error %.3g" % (got, want, abs(got - want) / want))
    assert float(st["nonfinite"]) == 0.0 and float(st["skipped"]) == 0.0      # nothing outside the operands (NaN all around them) was read
    assert abs(got - want) / want <= NORM_BAR
    assert torch.equal(first.view(torch.int32), second.view(torch.int32))      # no atomics: the same bits again
    assert float(st["clip_coef"]) == 1.0 and float(st["loss_scale"]) == 1.0


@pytest.mark.parametrize("grad_scale,double_step", [(1.0, False), (0.125, False), (1.0, True)], ids=["plain", "grad_scale_1_8", "double_step"])
def test_clipping_matches_torch(grad_scale, double_step):
    """Ten steps, max_norm at half of each step's norm; tensor LATE joins at step 3 (its own device step count) in every variant."""
    from dcvgan_amd import optim
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(7)
    guard = optim.GradGuard(max_norm=1.0)
    ref, hip, topt, hopt = _pair(gen, dev, guard)
    hopt.grad_scale = grad_scale
    worst = 0.0
    for step in range(1, 11):
        gs = []
        for i, (p, q) in enumerate(zip(ref, hip)):
            if i == LATE and step < 3:
                p.grad = None; q.grad = None
                continue
            g = _draw(p.shape, gen)
            gs.append((p, g))
            q.grad = _banded(g / grad_scale, dev)       # the HIP side sees the un-averaged sum (exact for a power of two)
        norm = _norm64([g for _, g in gs])
        guard.max_norm = 0.5 * norm
        coef = min(1.0, guard.max_norm / (norm + 1e-6))      # fp64
        for p, g in gs:
            p.grad = g * torch.tensor(coef, dtype=torch.float32)
        guard.measure()
        topt.step(); hopt.step()
        if double_step:
            topt.step(); hopt.step()
        st = guard.stats()
        torch.cuda.synchronize()
        worst = max(worst, abs(float(st["grad_norm"]) - norm) / norm)
        assert abs(float(st["grad_norm"]) - norm) / norm <= NORM_BAR, step
        assert abs(float(st["clip_coef"]) - coef) <= 1e-6 and float(st["skipped"]) == 0.0, step
        _compare(topt, hopt, ref, hip, UPDATE_BAR, step)
    print("worst relative norm error over 10 steps: %.3g" % worst)
    assert hopt.state[hip[LATE]]["step"].data_ptr() != hopt.state[hip[0]]["step"].data_ptr()
    assert int(hopt.state[hip[LATE]]["step"].item()) == (16 if double_step else 8) and int(hopt.state[hip[0]]["step"].item()) == (20 if double_step else 10)


def test_nonfinite_step_is_skipped():
    from dcvgan_amd import optim
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(3)
    guard = optim.GradGuard()
    ref, hip, topt, hopt = _pair(gen, dev, guard)

    def good():
        for p, q in zip(ref, hip):
            g = _draw(p.shape, gen)
            p.grad = g.clone(); q.grad = _banded(g, dev)
        guard.measure()
        topt.step(); hopt.step()

    good(); good()
    _compare(topt, hopt, ref, hip, UPDATE_BAR, "before")
    before = [(q.detach().clone(), hopt.state[q]["exp_avg"].clone(), hopt.state[q]["exp_avg_sq"].clone(), hopt.state[q]["step"].clone()) for q in hip]
    for i, q in enumerate(hip):      # the bad step: torch never sees it
        g = _draw(q.shape, gen)
        if i == 11:
            g.view(-1)[5000] = float("inf")
        if i == 16:
            g.view(-1)[123457] = float("nan")
        q.grad = _banded(g, dev)
    guard.measure()
    hopt.step()
    torch.cuda.synchronize()
    st = guard.stats()
    assert float(st["skipped"]) == 1.0 and float(st["skipped_total"]) == 1.0 and float(st["nonfinite"]) == 2.0
    for q, (p0, m0, v0, s0) in zip(hip, before):
        assert torch.equal(q.detach(), p0) and torch.equal(hopt.state[q]["exp_avg"], m0) and torch.equal(hopt.state[q]["exp_avg_sq"], v0)
        assert torch.equal(hopt.state[q]["step"], s0) and int(s0.item()) == 2
    good()
    st = guard.stats()
    torch.cuda.synchronize()
    assert float(st["skipped"]) == 0.0 and float(st["skipped_total"]) == 1.0 and float(st["nonfinite"]) == 0.0
    _compare(topt, hopt, ref, hip, UPDATE_BAR, "after")
    # skip_nonfinite=False measures the same and lets the step through
    loose = optim.GradGuard(skip_nonfinite=False)
    q = torch.nn.Parameter(torch.ones(8, device=dev))
    o = optim.Adam([q], guard=loose, **HP)
    q.grad = torch.tensor([1.0, float("inf")] + [0.0] * 6, device=dev)
    loose.measure(); o.step()
    torch.cuda.synchronize()
    assert float(loose.stats()["nonfinite"]) == 1.0 and float(loose.stats()["skipped"]) == 0.0 and int(o.state[q]["step"].item()) == 1


def test_dynamic_scale_follows_torch_gradscaler():
    from dcvgan_amd import optim
    dev = torch.device("cuda:0")
    pattern = [0, 0, 0, 1, 0, 0, 1, 1, 0, 0, 0, 0]      # 1 = a non-finite gradient
    kw = dict(growth_factor=2.0, backoff_factor=0.5, growth_interval=3)
    scaler = torch.amp.GradScaler("cpu", init_scale=1024.0, **kw)
    p = torch.nn.Parameter(torch.ones(3))
    sgd = torch.optim.SGD([p], lr=0.1)
    guard = optim.GradGuard(loss_scale=1024.0, dynamic=True, **kw)
    q = torch.nn.Parameter(torch.ones(3, device=dev))
    o = optim.Adam([q], guard=guard, **HP)
    want, got, roots, steps = [], [], [], []
    for bad in pattern:
        scaler.scale(torch.zeros(1))
        p.grad = torch.ones(3) * (float("inf") if bad else 1.0)
        scaler.step(sgd); scaler.update()
        want.append(scaler.get_scale())
        q.grad = torch.ones(3, device=dev) * (float("inf") if bad else 1.0)
        guard.measure(); o.step()
        got.append(float(guard.stats()["loss_scale"]))
        roots.append(float(guard.root(None)))
        steps.append(int(o.state[q]["step"].item()))
    assert got == want and roots == want, (got, want)
    assert steps[-1] == len(pattern) - sum(pattern) and float(guard.stats()["skipped_total"]) == float(sum(pattern))


def test_loss_scale_invariance():
    """g * 2^16 under loss_scale = 2^16 is the run on g under scale 1, bit for bit (powers of two: every product is exact), clipping included."""
    from dcvgan_amd import optim
    dev = torch.device("cuda:0")
    runs = []
    for scale in (1.0, 65536.0):
        gen = torch.Generator().manual_seed(5)
        guard = optim.GradGuard(max_norm=20.0, loss_scale=scale)
        _, hip, _, hopt = _pair(gen, dev, guard)
        norms = []
        for step in range(10):
            for q in hip:
                q.grad = _banded(_draw(q.shape, gen) * scale, dev)
            assert float(guard.root(None)) == scale
            guard.measure(); hopt.step()
            norms.append(guard.state.clone())
        torch.cuda.synchronize()
        runs.append((hip, hopt, norms))
    (hip_a, opt_a, st_a), (hip_b, opt_b, st_b) = runs
    clipped = 0
    for a, b in zip(st_a, st_b):
        assert torch.equal(a[2:4], b[2:4]) and float(a[4]) == float(b[4]) * 65536.0      # norm and coefficient equal; the factor carries 1 / scale
        clipped += int(float(a[3]) < 1.0)
    assert 0 < clipped, "max_norm never bit: the clipped branch was not exercised"
    for a, b in zip(hip_a, hip_b):
        assert torch.equal(a.detach(), b.detach())
        assert torch.equal(opt_a.state[a]["exp_avg"], opt_b.state[b]["exp_avg"]) and torch.equal(opt_a.state[a]["exp_avg_sq"], opt_b.state[b]["exp_avg_sq"])
        assert torch.equal(opt_a.state[a]["step"], opt_b.state[b]["step"])


def test_no_host_wait_and_launch_counts():
    from dcvgan_amd import native, optim
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(9)
    guard = optim.GradGuard(max_norm=1.0)
    _, hip, _, hopt = _pair(gen, dev, guard)
    twin = [torch.nn.Parameter(q.detach().clone()) for q in hip]
    plain = optim.Adam(twin, **HP)
    grads = [[_banded(_draw(q.shape, gen), dev) for q in hip] for _ in range(4)]
    for step in range(3):      # tensor LATE joins at step 3: two step-count groups from then on; buffers and tables exist after these
        for i, (q, t) in enumerate(zip(hip, twin)):
            q.grad = t.grad = None if (i == LATE and step < 2) else grads[step][i]
        guard.measure(); hopt.step(); plain.step()
    for i, (q, t) in enumerate(zip(hip, twin)):
        q.grad = t.grad = grads[3][i]
    torch.cuda.synchronize()
    groups = len({hopt.state[q]["step"].data_ptr() for q in hip})
    assert groups == 2
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        c0 = native.launch_count()
        guard.measure()
        c1 = native.launch_count()
        hopt.step()
        c2 = native.launch_count()
        st = guard.stats()
        root = guard.root(None)
        plain.step()
        c3 = native.launch_count()
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    torch.cuda.synchronize()
    assert len(hip) == 30 and c1 - c0 <= 3, c1 - c0
    assert (c2 - c1) == (c3 - c2) + groups, (c2 - c1, c3 - c2)
    assert all(v.dim() == 0 and v.is_cuda for v in st.values()) and root.dim() == 0 and root.is_cuda
    assert sorted(st) == ["clip_coef", "grad_norm", "loss_scale", "nonfinite", "skipped", "skipped_total"]


# --------------------------------------------------------------------------------------------------------------------------------------------------------- #
# the training iteration
# --------------------------------------------------------------------------------------------------------------------------------------------------------- #
def _setup(width_div=8):
    dev = torch.device("cuda:0")
    cfg = rig.small_cfg(width_div=width_div)
    models, _ = rig.seeded_models(cfg, dev, cfg.seed, 1234)
    return (cfg, models) + rig.clip_pair(cfg, dev, cfg.seed, geo_channels=1)


def _runner(cfg, models, guard):
    from dcvgan_amd import trainer
    rig.share_rng(models, 1234)      # a fresh stream for every runner over these models
    opts = trainer.build_optimizers(cfg, models, guard=guard)
    return trainer.StepRunner(cfg, models, opts, trainer.build_loss(cfg)), opts


def _flat(models):
    return {n: [p.detach().clone() for p in m.parameters()] for n, m in models.items()}


def _guard_that_never_clips_changes_nothing(width_div):
    cfg, models, xc, xg = _setup(width_div)
    twin = copy.deepcopy(models)
    init = _flat(models)
    r_plain, _ = _runner(cfg, twin, None)
    r_guard, opts = _runner(cfg, models, {})
    out_p = [r_plain.step(xc, xg, 3 + it) for it in range(2)]
    out_g = [r_guard.step(xc, xg, 3 + it) for it in range(2)]
    torch.cuda.synchronize()
    assert set(out_g[0]) == set(out_p[0]) | {"grad_norm_dis", "grad_norm_gen", "skipped_dis", "skipped_gen"}
    for k in out_p[0]:
        assert torch.equal(out_g[0][k], out_p[0][k]), k      # a root cotangent of exactly 1.0, and the first update comes after the first losses
    worst = 0.0
    for n in models:
        for p0, pg, pp in zip(init[n], models[n].parameters(), twin[n].parameters()):
            dg, dp = (pg.detach() - p0).double(), (pp.detach() - p0).double()
            if float(dp.abs().max()) == 0.0:
                assert float(dg.abs().max()) == 0.0
                continue
            worst = max(worst, float((dg - dp).abs().max() / dp.abs().max()))
    print("worst relative difference of a parameter's movement, guarded against unguarded: %.3g" % worst)
    assert worst <= 1e-6
    for it in range(2):
        for ph in ("dis", "gen"):
            assert float(out_g[it]["skipped_" + ph]) == 0.0
            assert math.isfinite(float(out_g[it]["grad_norm_" + ph])) and float(out_g[it]["grad_norm_" + ph]) > 0.0
    for name in ("idis", "ggen"):
        st = opts[name].guard.stats()
        assert float(st["skipped_total"]) == 0.0 and float(st["nonfinite"]) == 0.0 and float(st["clip_coef"]) == 1.0


def test_iteration_with_idle_guard_equals_unguarded():
    _guard_that_never_clips_changes_nothing(8)


def test_iteration_with_idle_guard_bf16_channels_last():
    """The same on the bf16 channels-last data path (fp32 master gradients behind 16-bit activations), switched on the way tests/test_cl16_oracle_gpu.py does.
    Width / 4 here, not / 8: that path concatenates 8-channel-aligned slices, so the stems' ndf / 2 channels must be a multiple of 8 (tests/dp_worker.py runs its
    channels-last mode at / 4 for the same reason)."""
    from dcvgan_amd import ops_cl
    ops_cl.enable(True)
    try:
        _guard_that_never_clips_changes_nothing(4)
    finally:
        ops_cl.enable(False)


def test_iteration_clipped_against_host_reference():
    """max_norm at half the first measured norm of each phase.  guard.measure is wrapped to copy gradients, parameters and moments to the host first; the reference
    is torch.optim.Adam on the host from that state, fed the captured gradients times the fp64 clip coefficient."""
    cfg, models, xc, xg = _setup()
    runner, opts = _runner(cfg, models, {})
    phases = {"dis": ("idis", "vdis", "gdis"), "gen": ("ggen", "cgen")}
    lr = {n: opts[n].lr for n in opts}
    wd = {n: opts[n].weight_decay for n in opts}
    captured = {}

    def wrap(phase):
        guard = opts[phases[phase][0]].guard
        orig = guard.measure

        def measure():
            torch.cuda.synchronize()
            snap = {}
            for n in phases[phase]:
                o = opts[n]
                snap[n] = [(None if p.grad is None else p.grad.detach().cpu().clone(), p.detach().cpu().clone(),
                            None if p not in o.state else (int(o.state[p]["step"].item()), o.state[p]["exp_avg"].cpu().clone(), o.state[p]["exp_avg_sq"].cpu().clone()))
                           for p in o.params]
            norm = _norm64([g for n in snap for g, _, _ in snap[n] if g is not None])
            if guard.max_norm is None:
                guard.max_norm = 0.5 * norm
            captured[phase] = (snap, norm, guard.max_norm)
            orig()
        guard.measure = measure

    for ph in phases:
        wrap(ph)
    for it in range(2):
        out = runner.step(xc, xg, 3 + it)
        torch.cuda.synchronize()
        for ph, names in phases.items():
            snap, norm, max_norm = captured[ph]
            got = float(out["grad_norm_" + ph])
            print("iteration %d %s: grad_norm %.9g, fp64 %.9g (relative error %.3g), max_norm %.6g" % (it + 1, ph, got, norm, abs(got - norm) / norm, max_norm))
            assert abs(got - norm) / norm <= NORM_BAR, (it, ph)
            assert float(out["skipped_" + ph]) == 0.0
            coef = min(1.0, max_norm / (norm + 1e-6))
            assert it > 0 or coef < 0.51
            for n in names:
                ref, have = [], []
                for (g, p0, s0), q in zip(snap[n], opts[n].params):
                    if g is None:
                        assert torch.equal(q.detach().cpu(), p0), n
                        continue
                    p = torch.nn.Parameter(p0.clone())
                    p.grad = g * torch.tensor(coef, dtype=torch.float32)
                    ref.append((p, s0)); have.append(q)
                topt = torch.optim.Adam([p for p, _ in ref], lr=lr[n], betas=(0.5, 0.999), eps=1e-8, weight_decay=wd[n])
                for p, s0 in ref:
                    if s0 is not None:
                        topt.state[p] = {"step": torch.tensor(float(s0[0])), "exp_avg": s0[1].clone(), "exp_avg_sq": s0[2].clone()}
                topt.step()
                if n == "ggen":      # stepped twice on one measurement
                    topt.step()
                for (p, _), q in zip(ref, have):
                    sh = opts[n].state[q]
                    assert int(topt.state[p]["step"]) == int(sh["step"].item()), n
                    assert _rel(q.detach(), p.detach()) <= UPDATE_BAR, (it, n, "p")
                    assert _rel(sh["exp_avg"], topt.state[p]["exp_avg"]) <= UPDATE_BAR, (it, n, "m")
                    assert _rel(sh["exp_avg_sq"], topt.state[p]["exp_avg_sq"]) <= UPDATE_BAR, (it, n, "v")
