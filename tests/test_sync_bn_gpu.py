"""GPU, one process: synchronised BatchNorm through the C ABI (dcv_bn_sync_*), with the "ranks" played by slices of one batch along N, and through
ops.sync_bn_act / optim.sync_batchnorm at world 1 (force).

Reference: torch fp64 F.batch_norm on the host over the WHOLE batch.  Metric and bars are tests/test_ops_gpu.py::test_bn_act's: rel() < 1e-3 on outputs and
gradients, < 1e-5 on the running statistics.  Every case prints its worst figures (pytest -s) — they are recorded in DESIGN §7a."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
TOL, TOL_STATS = 1e-3, 1e-5


def rel(a, b):
    a = a.detach().double().cpu(); b = b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


@pytest.fixture(scope="module")
def dev():
    from dcvgan_amd import native
    native.lib()
    return torch.device("cuda:0")


def host_reference(x, gamma, beta, rm, rv, mask, act, slope, cot, eps=1e-5, momentum=0.1):
    """fp64 on the host over the whole batch -> y, (dx, dgamma, dbeta), running_mean, running_var"""
    x, gamma, beta = (t.detach().double().cpu().requires_grad_(True) for t in (x, gamma, beta))
    rm, rv = rm.double().cpu().clone(), rv.double().cpu().clone()
    h = F.batch_norm(x, rm, rv, gamma, beta, True, momentum, eps)
    if mask is not None:
        h = h * mask.double().cpu().view(x.shape[0], x.shape[1], *([1] * (x.dim() - 2)))
    y = F.leaky_relu(h, slope) if act else h
    gr = torch.autograd.grad((y * cot.double().cpu()).sum(), [x, gamma, beta])
    return y.detach(), gr, rm, rv


def off_the_kink(x, gamma, beta, margin=1e-4, eps=1e-5):
    """LeakyReLU is not differentiable at 0, and fp64 on the host and fp32 on the device need not land on the same side of it: a pre-activation of 5e-8 on the host is
    +3e-8 in fp32 (one fused multiply-add of values near 1, rounding 6e-8), and the two gradients then differ by 0.8 * dy at that element — a property of the test point,
    not an error of either side.  One such element among 147 456 moves rel(dx) to 3e-3.  So no test input may sit within fp32 rounding of the kink: elements whose fp64
    pre-activation is below `margin` (1e-4: a thousand roundings) are moved by 0.01 in x, about 0.006 in z.  The bars, the shapes and the reference stay as they are."""
    for _ in range(4):
        z = F.batch_norm(x.double(), None, None, gamma.double(), beta.double(), True, 0.0, eps)
        near = z.abs() < margin
        if not bool(near.any()):
            return x
        x = torch.where(near, x + 0.01, x)
    raise AssertionError("could not move the test input off the activation's kink")


def abi_sync_bn(dev, xs, ys, gamma, beta, rm0, rv0, masks, act, slope, cots, partials=None, eps=1e-5, momentum=0.1):
    """Every "rank" r owns xs[r] (device views): rows -> table -> finalize -> apply -> backward sums -> table -> backward apply.  Returns per-rank results."""
    from dcvgan_amd import native as N
    from dcvgan_amd.native import dims5, ptr, stream_ptr
    L = N.lib()
    world, Cn = len(xs), xs[0].shape[1]
    n = L.dcv_bn_sync_row_doubles(Cn)
    assert n == 2 * Cn + 1
    need = L.dcv_bn_workspace_bytes(Cn)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    rows = torch.zeros(world, n, dtype=torch.float64, device=dev)
    for r, x in enumerate(xs):
        xd = dims5(x)
        stat, nparts, pitch = partials[r] if partials is not None else (None, 0, 0)
        N.check(L.dcv_bn_sync_sums(ptr(x), C.byref(xd), ptr(stat), nparts, pitch, ptr(rows[r]), ptr(ws), need, stream_ptr()), "dcv_bn_sync_sums")
    out = []
    for r, (x, y) in enumerate(zip(xs, ys)):
        rm, rv, nbt = rm0.clone(), rv0.clone(), torch.zeros((), dtype=torch.int64, device=dev)
        stats = torch.full((2, Cn), float("nan"), device=dev)
        N.check(L.dcv_bn_sync_finalize(ptr(rows), world, Cn, eps, momentum, ptr(rm), ptr(rv), ptr(nbt), ptr(stats[0]), ptr(stats[1]), stream_ptr()), "dcv_bn_sync_finalize")
        xd, yd = dims5(x), dims5(y)
        N.check(L.dcv_bn_apply(ptr(x), C.byref(xd), ptr(y), C.byref(yd), ptr(gamma), ptr(beta), ptr(stats[0]), ptr(stats[1]), ptr(masks[r]), act, slope, stream_ptr()),
                "dcv_bn_apply")
        out.append(dict(y=y, rm=rm, rv=rv, nbt=nbt, stats=stats))
    brows = torch.zeros(world, n, dtype=torch.float64, device=dev)
    for r, x in enumerate(xs):
        xd, dyd = dims5(x), dims5(cots[r])
        N.check(L.dcv_bn_sync_backward_sums(ptr(cots[r]), C.byref(dyd), ptr(x), C.byref(xd), ptr(gamma), ptr(beta), ptr(out[r]["stats"][0]), ptr(out[r]["stats"][1]),
                                            ptr(masks[r]), act, slope, ptr(brows[r]), ptr(ws), need, stream_ptr()), "dcv_bn_sync_backward_sums")
    for r, x in enumerate(xs):
        dx = torch.full(x.shape, float("nan"), device=dev)
        dgb = torch.full((2, Cn), float("nan"), device=dev)
        xd, dyd, dxd = dims5(x), dims5(cots[r]), dims5(dx)
        N.check(L.dcv_bn_sync_backward_apply(ptr(cots[r]), C.byref(dyd), ptr(x), C.byref(xd), ptr(dx), C.byref(dxd), ptr(gamma), ptr(beta),
                                             ptr(out[r]["stats"][0]), ptr(out[r]["stats"][1]), ptr(masks[r]), act, slope, ptr(brows), world, r,
                                             ptr(dgb[0]), ptr(dgb[1]), ptr(ws), need, stream_ptr()), "dcv_bn_sync_backward_apply")
        out[r].update(dx=dx, dgamma=dgb[0], dbeta=dgb[1])
    torch.cuda.synchronize()
    return out


def check_against_host(out, ref, world_label):
    y_ref, (dx_ref, dg_ref, db_ref), rm_ref, rv_ref = ref
    y = torch.cat([o["y"] for o in out]); dx = torch.cat([o["dx"] for o in out])
    dg = sum(o["dgamma"].double() for o in out); db = sum(o["dbeta"].double() for o in out)
    fig = dict(y=rel(y, y_ref), dx=rel(dx, dx_ref), dgamma=rel(dg, dg_ref), dbeta=rel(db, db_ref),
               running_mean=max(rel(o["rm"], rm_ref) for o in out), running_var=max(rel(o["rv"], rv_ref) for o in out))
    print(f"sync-bn {world_label}: " + " ".join(f"{k}={v:.3g}" for k, v in fig.items()))
    assert not torch.isnan(dx).any() and not torch.isnan(y).any()
    for k in ("y", "dx", "dgamma", "dbeta"):
        assert fig[k] < TOL, fig
    assert fig["running_mean"] < TOL_STATS and fig["running_var"] < TOL_STATS, fig
    for o in out:
        assert int(o["nbt"]) == 1
        # every rank adds the same table in the same order: the same bits
        assert torch.equal(o["stats"], out[0]["stats"]) and torch.equal(o["rm"], out[0]["rm"]) and torch.equal(o["rv"], out[0]["rv"])
    return fig


# (shape, split along N, channel slice of a wider buffer: (total channels, first channel) or None)
CASES = [
    ((3, 6, 8, 8), (2, 1), None),
    ((2, 5, 4, 6, 6), (1, 1), None),
    ((4, 7, 1, 1), (3, 1), None),            # a rank with one value per channel, global N = 4
    ((2, 3, 5, 3, 3), (1, 1), None),
    ((12, 3, 64, 64), (8, 4), None),         # beyond the small-layer bound, split > 1, rows-kernel layout
    ((4, 6, 8, 8), (2, 2), (10, 4)),         # x and y: the second channel slice of a 10-channel buffer
]


@pytest.mark.parametrize("mode", ["train", "dropout", "none"])
@pytest.mark.parametrize("shape,split,view", CASES, ids=[f"{'x'.join(map(str, s))}_as_{'+'.join(map(str, p))}{'_slice' if v else ''}" for s, p, v in CASES])
def test_sync_bn_abi_slices_equal_whole_batch(dev, shape, split, view, mode):
    from dcvgan_amd import ops
    g = torch.Generator().manual_seed(11)
    Cn = shape[1]
    x = torch.randn(shape, generator=g) * 1.7 + 0.4
    gamma = torch.rand(Cn, generator=g) + 0.5; beta = torch.randn(Cn, generator=g)
    rm, rv = torch.randn(Cn, generator=g) * 0.1, torch.rand(Cn, generator=g) + 0.5
    cot = torch.randn(shape, generator=g)
    mask = (torch.rand(shape[0], Cn, generator=g) > 0.5).float() * 2.0 if mode == "dropout" else None
    x = off_the_kink(x, gamma, beta)
    act, slope = (ops.ACT_NONE, 0.0) if mode == "none" else (ops.ACT_LEAKY, 0.2)
    ref = host_reference(x, gamma, beta, rm, rv, mask, act != ops.ACT_NONE, slope, cot)
    if view is None:
        xb, yb = x.to(dev), torch.full(shape, float("nan"), device=dev)
    else:
        total, c0 = view
        wide = (shape[0], total) + tuple(shape[2:])
        xbuf, ybuf = torch.full(wide, 7.0, device=dev), torch.full(wide, float("nan"), device=dev)
        xb, yb = xbuf[:, c0:c0 + Cn], ybuf[:, c0:c0 + Cn]
        xb.copy_(x.to(dev))
    cot_d = cot.to(dev)
    bounds = [sum(split[:i]) for i in range(len(split) + 1)]
    sl = [slice(a, b) for a, b in zip(bounds[:-1], bounds[1:])]
    masks = [None if mask is None else mask[s].contiguous().to(dev) for s in sl]
    out = abi_sync_bn(dev, [xb[s] for s in sl], [yb[s] for s in sl], gamma.to(dev), beta.to(dev), rm.to(dev), rv.to(dev), masks, act, slope,
                      [cot_d[s] for s in sl])
    check_against_host(out, ref, f"{shape} as {split} {mode}")
    if view is not None:      # nothing outside the slice was touched
        assert bool(torch.isnan(ybuf[:, :view[1]]).all()) and bool((xbuf[:, :view[1]] == 7.0).all())


def test_sync_bn_kernel_notes_and_layouts(dev):
    """The large case takes the rows-kernel layout with more than one block per channel; each entry leaves a note for dcv_debug_last_kernel."""
    from dcvgan_amd import native as N
    from dcvgan_amd.native import dims5, ptr, stream_ptr
    L = N.lib()
    x = torch.randn(8, 3, 64, 64, device=dev)
    need = L.dcv_bn_workspace_bytes(3)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    row = torch.zeros(1, 7, dtype=torch.float64, device=dev)
    xd = dims5(x)
    N.check(L.dcv_bn_sync_sums(ptr(x), C.byref(xd), None, 0, 0, ptr(row), ptr(ws), need, stream_ptr()), "sums")
    note = L.dcv_debug_last_kernel().decode()
    assert "bn_stats_kernel<4> x 8 blocks per channel" in note and "bn_sync_fold_kernel" in note, note
    assert float(row[0, 6]) == 8 * 64 * 64
    assert rel(row[0, :3], x.double().sum((0, 2, 3))) < 1e-6 and rel(row[0, 3:6], (x.double() ** 2).sum((0, 2, 3))) < 1e-6
    stats = torch.empty(2, 3, device=dev)
    N.check(L.dcv_bn_sync_finalize(ptr(row), 1, 3, 1e-5, 0.1, None, None, None, ptr(stats[0]), ptr(stats[1]), stream_ptr()), "finalize")
    assert "bn_sync_finalize_kernel" in L.dcv_debug_last_kernel().decode()
    gamma, beta = torch.ones(3, device=dev), torch.zeros(3, device=dev)
    N.check(L.dcv_bn_sync_backward_sums(ptr(x), C.byref(xd), ptr(x), C.byref(xd), ptr(gamma), ptr(beta), ptr(stats[0]), ptr(stats[1]), None, 0, 0.0, ptr(row), ptr(ws), need,
                                        stream_ptr()), "backward sums")
    assert "bn_bwd_reduce_rows_kernel x 8 blocks per channel" in L.dcv_debug_last_kernel().decode(), L.dcv_debug_last_kernel().decode()
    dx, dgb = torch.empty_like(x), torch.empty(2, 3, device=dev)
    N.check(L.dcv_bn_sync_backward_apply(ptr(x), C.byref(xd), ptr(x), C.byref(xd), ptr(dx), C.byref(xd), ptr(gamma), ptr(beta), ptr(stats[0]), ptr(stats[1]), None, 0, 0.0,
                                         ptr(row), 1, 0, ptr(dgb[0]), ptr(dgb[1]), ptr(ws), need, stream_ptr()), "backward apply")
    assert "bn_sync_bwd_coef_kernel" in L.dcv_debug_last_kernel().decode()
    torch.cuda.synchronize()


def test_sync_bn_from_conv_epilogue_partials(dev):
    """Two "ranks" each run conv -> BatchNorm with the convolution's epilogue partials (ops.conv(..., bn_stats=[])) feeding dcv_bn_sync_sums; the reference is the
    host's fp64 BatchNorm over both ranks' convolution outputs."""
    from dcvgan_amd import ops
    g = torch.Generator().manual_seed(3)
    cin, cout, n = 16, 40, 96
    w = (torch.randn(cout, cin, 4, 4, generator=g) * 0.1).to(dev)
    geom = ops.conv_geom(w, (2, 2), (1, 1), False)
    ys, parts = [], []
    for r in range(2):
        box = []
        ys.append(ops.conv(torch.randn(n, cin, 64, 64, generator=g).to(dev), w, geom, bn_stats=box).detach())
        assert box, "this convolution is expected to leave BatchNorm partials"
        parts.append(box[0])
    gamma = torch.rand(cout, generator=g) + 0.5; beta = torch.randn(cout, generator=g)
    rm, rv = torch.zeros(cout), torch.ones(cout)
    cots = [torch.cos(torch.arange(y.numel(), dtype=torch.float32) * (0.37 + r)).view(y.shape) for r, y in enumerate(ys)]
    ref = host_reference(torch.cat(ys), gamma, beta, rm, rv, None, True, 0.2, torch.cat(cots))
    out = abi_sync_bn(dev, ys, [torch.empty_like(y) for y in ys], gamma.to(dev), beta.to(dev), rm.to(dev), rv.to(dev), [None, None], ops.ACT_LEAKY, 0.2,
                      [c.to(dev) for c in cots], partials=parts)
    check_against_host(out, ref, "conv-epilogue partials 96+96")
    own = abi_sync_bn(dev, ys, [torch.empty_like(y) for y in ys], gamma.to(dev), beta.to(dev), rm.to(dev), rv.to(dev), [None, None], ops.ACT_LEAKY, 0.2,
                      [c.to(dev) for c in cots])
    assert rel(out[0]["stats"], own[0]["stats"]) < 1e-6      # the partials and the op's own pass describe the same tensor


@pytest.mark.parametrize("shape", [(3, 6, 8, 8), (12, 3, 64, 64), (40, 32, 4, 4)])
def test_world_one_force_equals_local_batchnorm(dev, shape):
    """ops.sync_bn_act at world 1 (force) against ops.bn_act on the same input: both within the bars of the host, and close to one another."""
    from dcvgan_amd import ops, optim
    grp = optim.SyncBnGroup(force=True)
    assert grp.world == 1 and grp.active
    g = torch.Generator().manual_seed(5)
    Cn = shape[1]
    x = torch.randn(shape, generator=g) * 1.3 - 0.2
    gamma = torch.rand(Cn, generator=g) + 0.5; beta = torch.randn(Cn, generator=g)
    rm, rv = torch.randn(Cn, generator=g) * 0.1, torch.rand(Cn, generator=g) + 0.5
    cot = torch.randn(shape, generator=g)
    x = off_the_kink(x, gamma, beta)
    ref = host_reference(x, gamma, beta, rm, rv, None, True, 0.2, cot)
    res = []
    for sync in (True, False):
        xd = x.to(dev).requires_grad_(True)
        gd, bd = gamma.to(dev).requires_grad_(True), beta.to(dev).requires_grad_(True)
        rm_d, rv_d, nbt = rm.to(dev), rv.to(dev), torch.zeros((), dtype=torch.int64, device=dev)
        if sync:
            y = ops.sync_bn_act(xd, gd, bd, rm_d, rv_d, True, ops.ACT_LEAKY, 0.2, num_batches_tracked=nbt, group=grp)
        else:
            y = ops.bn_act(xd, gd, bd, rm_d, rv_d, True, ops.ACT_LEAKY, 0.2, num_batches_tracked=nbt)
        dx, dg, db = torch.autograd.grad((y * cot.to(dev)).sum(), [xd, gd, bd])
        out = [dict(y=y.detach(), dx=dx, dgamma=dg, dbeta=db, rm=rm_d, rv=rv_d, nbt=nbt, stats=torch.zeros(1))]
        check_against_host(out, ref, f"world 1 {'force' if sync else 'local'} {shape}")
        res.append(out[0])
    for k in ("y", "dx", "dgamma", "dbeta"):
        assert rel(res[0][k], res[1][k]) < TOL
    assert grp.collectives == 0


def test_short_workspace_is_refused_before_any_launch(dev):
    from dcvgan_amd import native as N
    from dcvgan_amd.native import dims5, ptr, stream_ptr
    L = N.lib()
    x = torch.randn(2, 4, 8, 8, device=dev)
    xd = dims5(x)
    need = L.dcv_bn_workspace_bytes(4)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    rows = torch.zeros(2, 9, dtype=torch.float64, device=dev)
    v = torch.ones(4, device=dev)
    n0 = N.launch_count()
    assert L.dcv_bn_sync_sums(ptr(x), C.byref(xd), None, 0, 0, ptr(rows[0]), ptr(ws), need - 1, stream_ptr()) == N.DCV_EWORKSPACE
    assert L.dcv_bn_sync_sums(ptr(x), C.byref(xd), None, 0, 0, ptr(rows[0]), None, need, stream_ptr()) == N.DCV_EWORKSPACE
    assert L.dcv_bn_sync_backward_sums(ptr(x), C.byref(xd), ptr(x), C.byref(xd), ptr(v), ptr(v), ptr(v), ptr(v), None, 0, 0.0, ptr(rows[0]), ptr(ws), need - 1,
                                       stream_ptr()) == N.DCV_EWORKSPACE
    assert L.dcv_bn_sync_backward_apply(ptr(x), C.byref(xd), ptr(x), C.byref(xd), ptr(x), C.byref(xd), ptr(v), ptr(v), ptr(v), ptr(v), None, 0, 0.0, ptr(rows), 2, 0,
                                        ptr(v), ptr(v), ptr(ws), need - 1, stream_ptr()) == N.DCV_EWORKSPACE
    assert b"workspace" in L.dcv_last_error()
    # bad arguments: no row, a rank outside the world, a pitch below the channel count, an empty table
    assert L.dcv_bn_sync_sums(ptr(x), C.byref(xd), None, 0, 0, None, ptr(ws), need, stream_ptr()) == N.DCV_EINVAL
    assert L.dcv_bn_sync_sums(ptr(x), C.byref(xd), ptr(x), 1, 3, ptr(rows[0]), ptr(ws), need, stream_ptr()) == N.DCV_EINVAL
    assert L.dcv_bn_sync_finalize(ptr(rows), 0, 4, 1e-5, 0.1, None, None, None, ptr(v), ptr(v), stream_ptr()) == N.DCV_EINVAL
    assert L.dcv_bn_sync_backward_apply(ptr(x), C.byref(xd), ptr(x), C.byref(xd), ptr(x), C.byref(xd), ptr(v), ptr(v), ptr(v), ptr(v), None, 0, 0.0, ptr(rows), 2, 2,
                                        ptr(v), ptr(v), ptr(ws), need, stream_ptr()) == N.DCV_EINVAL
    assert N.launch_count() == n0


def _bn_block(dev, cn=8):
    import torch.nn as nn
    torch.manual_seed(2)
    return nn.Sequential(nn.BatchNorm2d(cn), nn.LeakyReLU(0.2)).to(dev)


def test_eval_mode_of_a_marked_module_adds_no_launch(dev):
    from dcvgan_amd import layers, native, optim
    from dcvgan_amd.rng import PhiloxRng
    x = torch.randn(4, 8, 8, 8, device=dev)
    counts, outs = [], []
    for marked in (False, True):
        seq = _bn_block(dev).eval()
        grp = optim.sync_batchnorm(seq, force=True) if marked else None
        n0 = native.launch_count()
        outs.append(layers.run(seq, x, PhiloxRng(1)))
        counts.append(native.launch_count() - n0)
        assert grp is None or grp.collectives == 0
    assert counts[0] == counts[1] and torch.equal(outs[0], outs[1]), counts
    # ... while in training mode the marked module does take the sync route (its kernels leave their note), and an unmarked one again does not
    seq = _bn_block(dev).train()
    optim.sync_batchnorm(seq, force=True)
    layers.run(seq, x, PhiloxRng(1))
    n0 = native.launch_count()
    y = layers.run(seq, x.clone().requires_grad_(True), PhiloxRng(1))
    assert native.launch_count() - n0 == 4      # statistics pass, fold, finalize, apply
    n0 = native.launch_count()
    y.sum().backward()      # (autograd's thread: the kernel note is per thread, the launch count is not)
    assert native.launch_count() - n0 == 4      # reduce, fold, coefficients, apply
    optim.unsync_batchnorm(seq)
    assert optim.sync_bn_group_of(seq) is None
    n0 = native.launch_count()
    layers.run(seq, x, PhiloxRng(1))
    assert native.launch_count() - n0 <= 3


def test_marked_module_refuses_the_16_bit_channels_last_path(dev):
    from dcvgan_amd import layers, native, ops_cl, optim
    from dcvgan_amd.rng import PhiloxRng
    seq = _bn_block(dev).train()
    optim.sync_batchnorm(seq, force=True)
    ops_cl.enable(True)
    try:
        x = ops_cl.from_f32(torch.randn(4, 8, 8, 8, device=dev))
        assert ops_cl.is_cl(x)
        n0 = native.launch_count()
        with pytest.raises(native.NativeError, match="fp32-path only"):
            layers.run(seq, x, PhiloxRng(1))
        assert native.launch_count() == n0
        seq.eval()                      # eval mode has nothing to synchronise: the 16-bit path runs as ever
        layers.run(seq, x, PhiloxRng(1))
    finally:
        ops_cl.enable(False)


def test_marked_colour_generator_takes_the_unfused_head_route(dev, monkeypatch):
    """A marked up_blocks[5] leaves its BnLink empty (the fused head backward would reduce over the local batch only), and the colour generator's forward / backward at
    width / 8, B = 2 stays within the bars of the unmarked run."""
    from dcvgan_amd import ops, optim, trainer
    from dcvgan_amd.configs import CONFIGS
    from dcvgan_amd.rng import PhiloxRng
    cfg = CONFIGS["isogd-depth"].scaled(batchsize=2, width_div=8)
    xs = (torch.rand(2, 1, 16, 64, 64, generator=torch.Generator().manual_seed(4)) * 2 - 1).to(dev)
    links = []

    class Link(ops.BnLink):
        __slots__ = ()

        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            links.append(self)
    monkeypatch.setattr(ops, "BnLink", Link)

    def run(marked):
        torch.manual_seed(9)
        cgen = trainer.build_models(cfg, dev)["cgen"]
        cgen._rng = PhiloxRng(3)
        cgen.train()
        if marked:
            optim.sync_batchnorm(cgen.up_blocks[5], force=True)
            assert sum(1 for m in cgen.modules() if "_dcv_sync_bn" in m.__dict__) == 1
            optim.sync_batchnorm(cgen, force=True)
        del links[:]
        y = cgen.forward_videos(xs)
        state = [(lk.deferred, lk.x is None) for lk in links]
        (y * torch.linspace(-1, 1, y.numel(), device=dev).view_as(y)).sum().backward()
        torch.cuda.synchronize()
        return y.detach(), {n: p.grad.detach().clone() for n, p in cgen.named_parameters()}, {n: b.detach().clone() for n, b in cgen.named_buffers()}, state

    y0, g0, b0, s0 = run(False)
    y1, g1, b1, s1 = run(True)
    assert s1 == [(False, True)], s1                 # neutralised: not deferred, nothing noted for the fused backward
    assert len(s0) == 1 and s0[0][1] is False, s0    # (the unmarked run does note the BatchNorm for the head)
    worst = max([rel(y1, y0)] + [rel(g1[n], g0[n]) for n in g0])
    worst_b = max(rel(b1[n], b0[n]) for n in b0 if b0[n].is_floating_point())
    print(f"sync-bn cgen width/8 B=2, marked (force) vs unmarked: outputs+gradients {worst:.3g}, running statistics {worst_b:.3g}")
    assert rel(y1, y0) < TOL
    for n in g0:
        assert rel(g1[n], g0[n]) < TOL, (n, rel(g1[n], g0[n]))
    for n in b0:
        if b0[n].is_floating_point():
            assert rel(b1[n], b0[n]) < TOL_STATS, n
        else:
            assert torch.equal(b1[n], b0[n]), n
