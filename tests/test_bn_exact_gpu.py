"""GPU: every BatchNorm kernel variant against the fp64 host reference, bit for bit where tests/exactbn.py proves that possible (integer-scheme operands, eps = 0)
and within a counted rounding bound elsewhere; called through the C ABI, every output pre-filled with NaN, every operand between two 8192-element NaN guard
bands, and every case asserting the note its entry point leaves for dcv_debug_last_kernel — so a case cannot land on another branch when a threshold moves.

fp32 NCDHW: small / stats<VEC> x split / rows kernels, vec 1 by odd plane, pointer or stride, non-contiguous planes, the generators' permuted layout, channel
slices, the 8192-block grid-stride; the raw fp64 sums through dcv_bn_sync_sums / dcv_bn_sync_backward_sums; the partials finalisers; the Tanh branch.
16-bit channels-last: every group count's combine scheme (xor tree G = 1 .. 64, serial chain incl. G = 128 with 64 KB of LDS), idle tail threads, 3-D pixels,
fewer pixels than slots, the 1024-block cap, channel slices.  A real-valued companion per case checks eps, rsqrt and general-position arithmetic.

Not covered here: the apply grid's 8192-block cap of the channels-last path needs more than 65536 * pb pixels — too large for a test of a few seconds; it is left
to the workload-size tests (tests/test_b70_gpu.py, tests/test_b100_gpu.py).  Nor is the fold of the fp32 runs in the channels-last reductions triggered
(run == 16 in cl_bn_stats_kernel, run == 32 in cl_bn_bwd_reduce_kernel: they need 64 pixels per thread), nor mean / std ratios beyond those of the inputs used."""
import ctypes as C
import functools

import pytest
import torch

from tests import exactbn as X
from tests import rig

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from dcvgan_amd import native
    native.lib()
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _stop_after_fault():
    """After a device fault (seen here or anywhere else through tests/rig.py) nothing else of this module is started on the GPU"""
    rig.stop_after_fault()
    yield


sync = rig.sync


def note():
    from dcvgan_amd import native as N
    return N.lib().dcv_debug_last_kernel().decode()


@functools.lru_cache(maxsize=2)
def exact_operands(name, shape):
    return X.exact_operands(name, shape)


@functools.lru_cache(maxsize=2)
def real_operands(name, shape, bf16):
    return X.real_operands(name, shape, bf16)


def act_code(mode):
    from dcvgan_amd import native as N
    return {"leaky": N.ACT_LEAKY, "none": N.ACT_NONE, "tanh": N.ACT_TANH}[X.act_of(mode)[1]]


def bits_equal(a, b):
    it = {4: torch.int32, 2: torch.int16}[a.element_size()]
    return bool(torch.equal(a.view(it), b.view(it)))


HALF = 0.5 + 2.0 ** -20      # a quantity computed in fp64 (error far below 2^-20 fp32 ulps) and stored as fp32: half an ulp


# ------------------------------------------------------------------------------------------------------------------------------------------------------
# the two paths behind one interface: operands in guarded storage, the entry points, the notes
# ------------------------------------------------------------------------------------------------------------------------------------------------------
class Path32:
    bf16 = False
    dtype = torch.float32

    def __init__(self, case):
        self.case, self.shape = case, case.shape
        self.d = X.dispatch32(case.shape, (case.layout,))
        self.run = X.RUN_SMALL if self.d.small else X.RUN32

    def tensor(self, dev, fill=None, body=float("nan")):
        return X.guarded(self.shape, self.case.layout, dev, fill=None if fill is None else fill.float(), body=body)

    def outside_intact(self, storage, before):
        return X.untouched_outside(storage, before, self.shape, self.case.layout)

    def owner(self, idx):
        return X.owner32(self.d, self.shape, idx)

    def ws(self, dev):
        from dcvgan_amd import native as N
        need = N.lib().dcv_bn_workspace_bytes(self.shape[1])
        return torch.empty(need, dtype=torch.uint8, device=dev), need

    forward_name, backward_name = "dcv_bn_act_forward", "dcv_bn_act_backward"

    def note_forward(self, training):
        return X.note_forward(self.d, training)

    def note_backward(self):
        return X.note_backward(self.d)

    def dx_exact(self, o, rb, training):
        return X.dx_exact(o, rb)

    def dx_bound(self, o, rb, training, **kw):
        return X.dx_bound(o, rb, **kw)


class PathCL:
    bf16 = True
    dtype = torch.bfloat16

    def __init__(self, case):
        self.case, self.shape = case, case.shape
        self.d = X.dispatch_cl(case.shape)
        self.run = X.RUN_CL
        self.pitch, self.c0 = (case.layout[1], case.layout[2]) if isinstance(case.layout, tuple) else (case.shape[1], 0)

    def _view(self, storage):
        n, c, sp = self.shape[0], self.shape[1], tuple(self.shape[2:])
        numel = storage.numel() - 2 * X.GUARD
        body = storage[X.GUARD:X.GUARD + numel].view((n,) + sp + (self.pitch,))
        return body.permute(*((0, len(sp) + 1) + tuple(range(1, len(sp) + 1))))[:, self.c0:self.c0 + c]

    def tensor(self, dev, fill=None, body=float("nan")):
        """Channels-last: element (n, pixel, c) at n PIX pitch + pixel pitch + c0 + c, between two NaN guard bands (tests/test_cl16_gpu.py::guarded_cl's layout, with a pitch)"""
        numel = self.shape[0] * self.pitch
        for s in self.shape[2:]:
            numel *= s
        storage = torch.full((numel + 2 * X.GUARD,), float("nan"), dtype=torch.bfloat16, device=dev)
        storage[X.GUARD:X.GUARD + numel] = body
        t = self._view(storage)
        if fill is not None:
            t.copy_(fill.to(torch.bfloat16))
        return t, storage

    def outside_intact(self, storage, before):
        a, b = storage.clone(), before.clone()
        self._view(a).zero_(); self._view(b).zero_()
        return bits_equal(a, b)

    def owner(self, idx):
        return X.owner_cl(self.d, self.shape, idx)

    def ws(self, dev):
        from dcvgan_amd import native as N
        need = N.lib().dcv_cl_bn_workspace_bytes(self.shape[1])
        return torch.empty(need, dtype=torch.uint8, device=dev), need

    forward_name, backward_name = "dcv_cl_bn_act_forward", "dcv_cl_bn_act_backward"

    def note_forward(self, training):
        return X.note_cl(self.d, "forward" if training else "eval")

    def note_backward(self):
        return X.note_cl(self.d, "backward")

    def dx_exact(self, o, rb, training):
        return X.cl_dx_exact(o, rb, training)

    def dx_bound(self, o, rb, training, **kw):
        kw.pop("ddz", None)
        return X.cl_dx_bound(o, rb, training=training, **kw)


def f32(dev, t):
    return None if t is None else t.float().to(dev).contiguous()


def forward(P, dev, o, mode, eps, momentum, slope, rm0, rv0):
    """One call of the forward entry on guarded operands -> dict of device results (x's and y's surroundings already checked)"""
    from dcvgan_amd import native as N
    from dcvgan_amd.native import dims5, ptr, stream_ptr
    L = N.lib()
    Cn = P.shape[1]
    x, xs = P.tensor(dev, fill=o.x, body=7.0)
    y, ys = P.tensor(dev)
    xs0, ys0 = xs.clone(), ys.clone()
    gamma, beta, rm, rv = f32(dev, o.gamma), f32(dev, o.beta), f32(dev, rm0), f32(dev, rv0)
    mask = f32(dev, o.mask) if X.act_of(mode)[0] else None
    nbt = torch.zeros((), dtype=torch.int64, device=dev)
    stats = torch.full((2, Cn), float("nan"), device=dev)
    ws, need = P.ws(dev)
    xd, yd = dims5(x), dims5(y)
    training = int(mode != "eval")
    N.check(getattr(L, P.forward_name)(ptr(x), C.byref(xd), ptr(y), C.byref(yd), ptr(gamma), ptr(beta), ptr(rm), ptr(rv), ptr(nbt), ptr(stats[0]), ptr(stats[1]), ptr(mask),
                                        training, momentum, eps, act_code(mode), slope, ptr(ws), need, stream_ptr()), P.forward_name)
    got = note()
    sync()
    assert got == P.note_forward(bool(training)), got
    assert bits_equal(xs, xs0), "the forward pass wrote to its input's storage"
    assert P.outside_intact(ys, ys0), "the forward pass wrote outside y (guard bands or the rest of the buffer)"
    return dict(y=y.cpu(), mean=stats[0].cpu(), invstd=stats[1].cpu(), rm=rm.cpu(), rv=rv.cpu(), nbt=int(nbt))


def backward(P, dev, o, mode, slope, save_mean, save_invstd):
    from dcvgan_amd import native as N
    from dcvgan_amd.native import dims5, ptr, stream_ptr
    L = N.lib()
    Cn = P.shape[1]
    x, xs = P.tensor(dev, fill=o.x, body=7.0)
    dy, dys = P.tensor(dev, fill=o.dy, body=7.0)
    dx, dxs = P.tensor(dev)
    xs0, dys0, dxs0 = xs.clone(), dys.clone(), dxs.clone()
    gamma, beta, sm, si = f32(dev, o.gamma), f32(dev, o.beta), f32(dev, save_mean), f32(dev, save_invstd)
    mask = f32(dev, o.mask) if X.act_of(mode)[0] else None
    dgb = torch.full((2, Cn), float("nan"), device=dev)
    ws, need = P.ws(dev)
    xd, dyd, dxd = dims5(x), dims5(dy), dims5(dx)
    N.check(getattr(L, P.backward_name)(ptr(dy), C.byref(dyd), ptr(x), C.byref(xd), ptr(dx), C.byref(dxd), ptr(gamma), ptr(beta), ptr(sm), ptr(si), ptr(mask),
                                         int(mode != "eval"), act_code(mode), slope, ptr(dgb[0]), ptr(dgb[1]), ptr(ws), need, stream_ptr()), P.backward_name)
    got = note()
    sync()
    assert got == P.note_backward(), got
    assert bits_equal(xs, xs0) and bits_equal(dys, dys0), "the backward pass wrote to its inputs' storage"
    assert P.outside_intact(dxs, dxs0), "the backward pass wrote outside dx (guard bands or the rest of the buffer)"
    return dict(dx=dx.cpu(), dgamma=dgb[0].cpu(), dbeta=dgb[1].cpu())


# ------------------------------------------------------------------------------------------------------------------------------------------------------
# the integer scheme
# ------------------------------------------------------------------------------------------------------------------------------------------------------
def check_exact_case(P, dev, mode):
    case = P.case
    o = exact_operands(case.name, case.shape)
    nd = len(case.shape)
    within = functools.partial(X.assert_within, shape=case.shape)
    mk = o.mask.view(o.mask.shape + (1,) * (nd - 2)) if X.act_of(mode)[0] else 1.0
    if mode == "eval":
        r = X.reference(o, mode)
        f = forward(P, dev, o, mode, 0.0, 0.5, X.SLOPE, o.rm, o.rv)
        assert bool(X.y_exact(o, r).all())
        within("save_mean", f["mean"], r.mean, 0.0); within("save_invstd", f["invstd"], r.invstd, 0.0)
        within("y", f["y"], r.y, 0.0, owner=P.owner, bf16=P.bf16)
        within("running_mean", f["rm"], o.rm, 0.0); within("running_var", f["rv"], o.rv, 0.0)
        assert f["nbt"] == 0
        rb, sm, si = r, o.rm, r.invstd
    else:
        r = X.reference(o, mode, rm0=o.rm, rv0=o.rv)
        f = forward(P, dev, o, mode, 0.0, 0.5, X.SLOPE, o.rm, o.rv)
        if X.stats_exact(o, r):
            assert bool(X.y_exact(o, r).all())
            bm = bi = brm = yb = 0.0
        else:       # an odd count: the +- balance cannot hold, mean and invstd are fp64 results rounded to fp32 and y carries their rounding
            bm, bi, brm = HALF * X.ulp32(r.mean), HALF * X.ulp32(r.invstd), X.ulp32(r.rm)
            yb = X.y_bound(o, r, dmean=bm, dis_rel=bi / r.invstd) * mk
        within("save_mean", f["mean"], r.mean, bm); within("save_invstd", f["invstd"], r.invstd, bi)
        within("y", f["y"], r.y, yb, owner=P.owner, bf16=P.bf16)
        within("running_mean", f["rm"], r.rm, brm)
        within("running_var", f["rv"], r.rv, X.ulp32(r.rv))        # the unbiased factor count / (count - 1) is inexact
        assert f["nbt"] == 1
        sm, si = o.m, 1.0 / o.a
        rb = X.reference(o, mode, mean=sm, invstd=si)
    assert X.sums_exact(o, rb, P.run, mode)
    b = backward(P, dev, o, mode, X.SLOPE, sm, si)
    within("dbeta", b["dbeta"], rb.dbeta, 0.0); within("dgamma", b["dgamma"], rb.dgamma, 0.0)
    training = mode != "eval"
    ex = P.dx_exact(o, rb, training)
    bound = torch.where(ex, torch.zeros_like(rb.dx), P.dx_bound(o, rb, training))
    within("dx", b["dx"], rb.dx, bound, owner=P.owner, bf16=P.bf16)


PAIRS32 = [(c, m) for c in X.CASES32 for m in X.MODES]
PAIRS_CL = [(c, m) for c in X.CASES_CL for m in X.MODES]


@pytest.mark.parametrize("case,mode", PAIRS32, ids=[f"{c.name}-{m}" for c, m in PAIRS32])
def test_bn_exact_fp32(dev, case, mode):
    check_exact_case(Path32(case), dev, mode)


@pytest.mark.parametrize("case,mode", PAIRS_CL, ids=[f"{c.name}-{m}" for c, m in PAIRS_CL])
def test_bn_exact_cl(dev, case, mode):
    check_exact_case(PathCL(case), dev, mode)


@pytest.mark.parametrize("case", X.CASES32, ids=lambda c: c.name)
def test_bn_raw_sums_fp32(dev, case):
    """The fp64 rows of bn_stats_kernel, bn_bwd_reduce_kernel and bn_bwd_reduce_rows_kernel, as dcv_bn_sync_sums / dcv_bn_sync_backward_sums expose them: the integers"""
    from dcvgan_amd import native as N
    from dcvgan_amd.native import dims5, ptr, stream_ptr
    L = N.lib()
    P = Path32(case)
    o = exact_operands(case.name, case.shape)
    Cn = case.shape[1]
    x, _ = P.tensor(dev, fill=o.x, body=7.0)
    dy, _ = P.tensor(dev, fill=o.dy, body=7.0)
    ws, need = P.ws(dev)
    rows = torch.full((2, 2 * Cn + 1), float("nan"), dtype=torch.float64, device=dev)
    xd, dyd = dims5(x), dims5(dy)
    gamma, beta, sm, si, mask_d = f32(dev, o.gamma), f32(dev, o.beta), f32(dev, o.m), f32(dev, 1.0 / o.a), f32(dev, o.mask)      # held: a temporary's memory is reused
    N.check(L.dcv_bn_sync_sums(ptr(x), C.byref(xd), None, 0, 0, ptr(rows[0]), ptr(ws), need, stream_ptr()), "dcv_bn_sync_sums")
    assert note() == X.note_sync_sums(P.d), note()
    for mode in ("dropout", "none"):
        rb = X.reference(o, mode, mean=o.m, invstd=1.0 / o.a)
        assert X.sums_exact(o, rb, X.RUN32, mode)
        mask = mask_d if mode == "dropout" else None
        N.check(L.dcv_bn_sync_backward_sums(ptr(dy), C.byref(dyd), ptr(x), C.byref(xd), ptr(gamma), ptr(beta), ptr(sm), ptr(si),
                                            ptr(mask), act_code(mode), X.SLOPE, ptr(rows[1]), ptr(ws), need, stream_ptr()), "dcv_bn_sync_backward_sums")
        assert note() == X.note_sync_backward_sums(P.d), note()
        sync()
        got = rows.cpu()
        X.assert_within("sum x", got[0, :Cn], rb.s0, 0.0, case.shape); X.assert_within("sum x^2", got[0, Cn:2 * Cn], rb.s1, 0.0, case.shape)
        X.assert_within("sum dz", got[1, :Cn], rb.sdz, 0.0, case.shape); X.assert_within("sum dz xhat", got[1, Cn:2 * Cn], rb.sdzx, 0.0, case.shape)
        assert float(got[0, 2 * Cn]) == rb.count and float(got[1, 2 * Cn]) == rb.count


# ------------------------------------------------------------------------------------------------------------------------------------------------------
# the partials finalisers: synthetic integer tables stat[nparts][pitch][2]
# ------------------------------------------------------------------------------------------------------------------------------------------------------
def partial_table(target0, target1, nparts, pitch, seed):
    """Integer partials whose column sums are the targets; the columns past the channel count hold NaN (a wrong pitch reads them)"""
    g = torch.Generator().manual_seed(seed)
    Cn = target0.numel()
    t = torch.full((nparts, pitch, 2), float("nan"), dtype=torch.float64)
    t[:, :Cn, 0] = torch.randint(-50, 51, (nparts, Cn), generator=g).double()
    t[:, :Cn, 1] = torch.randint(0, 61, (nparts, Cn), generator=g).double()
    t[-1, :Cn, 0] += target0 - t[:, :Cn, 0].sum(0)
    t[-1, :Cn, 1] += target1 - t[:, :Cn, 1].sum(0)
    assert bool(X.is_f32(t[:, :Cn]).all()) and float(t[:, :Cn].abs().max()) < 2 ** 24
    return t


@pytest.mark.parametrize("pitch_extra", [0, 3])
@pytest.mark.parametrize("nparts", [1, 255, 256, 257, 700])
def test_partials_finalisers(dev, nparts, pitch_extra):
    """bn_partials_finalize_kernel (through dcv_bn_forward_stats_only and dcv_bn_act_forward_stats) and cl_bn_finalize_stat_kernel: the p += 256 stride and the
    tree reduce, with column sums that are the integer scheme's sums — mean, invstd, running_mean and y exact."""
    from dcvgan_amd import native as N
    from dcvgan_amd.native import dims5, ptr, stream_ptr
    L = N.lib()
    for P in (Path32(X.Case("finalise32", (4, 5, 8, 8), "plain", {})), PathCL(X.Case("finalise_cl", (4, 40, 8, 8), "plain", {}))):
        shape, Cn = P.shape, P.shape[1]
        o = X.exact_operands(P.case.name, shape)
        r = X.reference(o, "leaky", rm0=o.rm, rv0=o.rv)
        assert X.stats_exact(o, r) and bool(X.y_exact(o, r).all())
        pitch = Cn + pitch_extra
        stat = partial_table(r.s0, r.s1, nparts, pitch, nparts * 8 + pitch_extra).float().to(dev)
        x, _ = P.tensor(dev, fill=o.x, body=7.0)
        y, ys = P.tensor(dev)
        ys0 = ys.clone()
        xd, yd = dims5(x), dims5(y)
        gamma, beta = f32(dev, o.gamma), f32(dev, o.beta)
        ws, need = P.ws(dev)

        def fresh():
            return f32(dev, o.rm), f32(dev, o.rv), torch.zeros((), dtype=torch.int64, device=dev), torch.full((2, Cn), float("nan"), device=dev)

        def check(rm, rv, nbt, stats):
            sync()
            X.assert_within("save_mean", stats[0], r.mean, 0.0, shape); X.assert_within("save_invstd", stats[1], r.invstd, 0.0, shape)
            X.assert_within("running_mean", rm, r.rm, 0.0, shape); X.assert_within("running_var", rv, r.rv, X.ulp32(r.rv), shape)
            assert int(nbt) == 1

        if not P.bf16:
            rm, rv, nbt, stats = fresh()
            N.check(L.dcv_bn_forward_stats_only(ptr(x), C.byref(xd), ptr(rm), ptr(rv), ptr(nbt), ptr(stats[0]), ptr(stats[1]), 0.5, 0.0, ptr(stat), nparts, pitch, stream_ptr()),
                    "dcv_bn_forward_stats_only")
            assert note() == f"bn_partials_finalize_kernel ({nparts} partials, pitch {pitch}), statistics only", note()
            check(rm, rv, nbt, stats)
        rm, rv, nbt, stats = fresh()
        name = "dcv_cl_bn_act_forward_stats" if P.bf16 else "dcv_bn_act_forward_stats"
        N.check(getattr(L, name)(ptr(x), C.byref(xd), ptr(y), C.byref(yd), ptr(gamma), ptr(beta), ptr(rm), ptr(rv), ptr(nbt), ptr(stats[0]), ptr(stats[1]), None,
                                 0.5, 0.0, act_code("leaky"), X.SLOPE, ptr(stat), nparts, pitch, ptr(ws), need, stream_ptr()), name)
        assert note() == (X.note_cl_stats(P.d, nparts, pitch) if P.bf16 else X.note_forward_stats(P.d, nparts, pitch)), note()
        check(rm, rv, nbt, stats)
        X.assert_within("y", y.cpu(), r.y, 0.0, shape, owner=P.owner, bf16=P.bf16)
        assert P.outside_intact(ys, ys0)
        if P.bf16:      # the channels-last entry can only refuse a table narrower than the channel count
            rc = L.dcv_cl_bn_act_forward_stats(ptr(x), C.byref(xd), ptr(y), C.byref(yd), ptr(gamma), ptr(beta), ptr(rm), ptr(rv), ptr(nbt), ptr(stats[0]), ptr(stats[1]), None,
                                               0.5, 0.0, act_code("leaky"), X.SLOPE, ptr(stat), nparts, Cn - 1, ptr(ws), need, stream_ptr())
            assert rc != 0


def test_forward_stats_small_layer_ignores_the_partials(dev):
    """A small-kernel shape handed partials computes its own sums in bn_fwd_small_kernel: a table of NaNs must not matter, and the note says so"""
    from dcvgan_amd import native as N
    from dcvgan_amd.native import dims5, ptr, stream_ptr
    L = N.lib()
    case = X.by_name(X.CASES32, "small_min")
    P = Path32(case)
    o = exact_operands(case.name, case.shape)
    r = X.reference(o, "leaky", rm0=o.rm, rv0=o.rv)
    Cn = case.shape[1]
    x, _ = P.tensor(dev, fill=o.x, body=7.0)
    y, ys = P.tensor(dev)
    stat = torch.full((3, Cn, 2), float("nan"), device=dev)
    rm, rv, nbt, stats = f32(dev, o.rm), f32(dev, o.rv), torch.zeros((), dtype=torch.int64, device=dev), torch.full((2, Cn), float("nan"), device=dev)
    ws, need = P.ws(dev)
    xd, yd = dims5(x), dims5(y)
    gamma, beta = f32(dev, o.gamma), f32(dev, o.beta)
    N.check(L.dcv_bn_act_forward_stats(ptr(x), C.byref(xd), ptr(y), C.byref(yd), ptr(gamma), ptr(beta), ptr(rm), ptr(rv), ptr(nbt), ptr(stats[0]), ptr(stats[1]),
                                       None, 0.5, 0.0, act_code("leaky"), X.SLOPE, ptr(stat), 3, Cn, ptr(ws), need, stream_ptr()), "dcv_bn_act_forward_stats")
    assert note() == X.note_forward_stats(P.d, 3, Cn), note()
    sync()
    X.assert_within("save_mean", stats[0], r.mean, 0.0, case.shape); X.assert_within("save_invstd", stats[1], r.invstd, 0.0, case.shape)
    X.assert_within("y", y.cpu(), r.y, 0.0, case.shape, owner=P.owner)
    assert int(nbt) == 1


def test_bn_apply_notes(dev):
    """dcv_bn_apply alone (saved statistics): the three apply kernels by shape, exact"""
    from dcvgan_amd import native as N
    from dcvgan_amd.native import dims5, ptr, stream_ptr
    L = N.lib()
    seen = set()
    for name in ("rows_3d", "gen4_split_a", "gen1_odd_a"):
        case = X.by_name(X.CASES32, name)
        P = Path32(case)
        o = exact_operands(case.name, case.shape)
        r = X.reference(o, "leaky", mean=o.m, invstd=1.0 / o.a)
        x, _ = P.tensor(dev, fill=o.x, body=7.0)
        y, ys = P.tensor(dev)
        ys0 = ys.clone()
        xd, yd = dims5(x), dims5(y)
        gamma, beta, sm, si = f32(dev, o.gamma), f32(dev, o.beta), f32(dev, o.m), f32(dev, 1.0 / o.a)
        N.check(L.dcv_bn_apply(ptr(x), C.byref(xd), ptr(y), C.byref(yd), ptr(gamma), ptr(beta), ptr(sm), ptr(si), None,
                               act_code("leaky"), X.SLOPE, stream_ptr()), "dcv_bn_apply")
        assert note() == f"BnApply {P.d.ew} (saved statistics)", note()
        seen.add(P.d.ew)
        sync()
        X.assert_within("y", y.cpu(), r.y, 0.0, case.shape, owner=P.owner)
        assert P.outside_intact(ys, ys0)
    assert seen == {"ew_rows", "ew<4>", "ew<1>"}


# ------------------------------------------------------------------------------------------------------------------------------------------------------
# real-valued companion: eps, rsqrt and general-position arithmetic, against derived elementwise bounds
# ------------------------------------------------------------------------------------------------------------------------------------------------------
EPS, MOMENTUM, SLOPE_REAL = 1e-5, 0.1, 0.2
# tanhf: the device library follows OpenCL's accuracy requirements (ROCm device-libs, doc/OCML.md); the OpenCL C specification, "Relative error as ULPs", gives
# tanh <= 5 ulp in single precision.  One fp32 ulp is at most 2 U relative.
TANH_ULPS = 5


def check_real_case(P, dev, mode):
    case = P.case
    o = real_operands(case.name, case.shape, P.bf16)
    nd = len(case.shape)
    dims = (0,) + tuple(range(2, nd))
    pc = lambda v: X.per_channel(v, nd)
    U = X.U
    tanh = mode == "tanh"
    slope = 0.0 if tanh else SLOPE_REAL
    mk = o.mask.view(o.mask.shape + (1,) * (nd - 2)) if X.act_of(mode)[0] else torch.ones(())
    r = X.reference(o, mode, eps=EPS, momentum=MOMENTUM, slope=slope, rm0=o.rm, rv0=o.rv)
    f = forward(P, dev, o, mode, EPS, MOMENTUM, slope, o.rm, o.rv)
    bm, bv, dmean, dis, dvar = X.stat_bounds(o, r, P.run, EPS)
    fig = {}

    def ratio(name, got, want, bound, owner=None):
        fig[name] = X.assert_within(f"{case.name} {mode} {name}", got, want, bound, case.shape, owner=owner)

    ratio("mean", f["mean"], r.mean, bm)                                                   # |mean - mean64| <= L 2^-24 mean|x|
    ratio("var", 1.0 / f["invstd"].double() ** 2 - EPS, r.var, bv)                         # |var - var64| <= L 2^-24 mean(x^2), var read back from save_invstd
    half16 = (2.0 ** -8) if P.bf16 else 0.0                                                # half a bf16 ulp of the stored result
    zb = X.y_bound(o, r, dmean=dmean, dis_rel=dis, roundings=6) * mk
    yb = zb + (TANH_ULPS * 2 * U * r.y.abs() if tanh else 0.0) + half16 * r.y.abs()
    ratio("y", f["y"], r.y, yb, P.owner)
    cnt = r.count
    ratio("running_mean", f["rm"], r.rm, MOMENTUM * bm + 3 * U * ((1 - MOMENTUM) * o.rm.abs() + MOMENTUM * r.mean.abs()))
    ratio("running_var", f["rv"], r.rv, MOMENTUM * dvar * cnt / (cnt - 1) + 3 * U * ((1 - MOMENTUM) * o.rv.abs() + MOMENTUM * r.var * cnt / (cnt - 1)))
    assert f["nbt"] == 1
    # the backward pass is handed the reference's statistics rounded to fp32, and the reference uses those very values
    sm, si = r.mean.float().double(), r.invstd.float().double()
    rb = X.reference(o, mode, eps=EPS, mean=sm, invstd=si, slope=slope)
    b = backward(P, dev, o, mode, slope, sm, si)
    ddz = None
    if tanh:      # dz = dy (1 - t^2), t = tanhf(z'): z' within the apply expression's roundings of z, t within TANH_ULPS of tanh(z'), two roundings on 1 - t t
        dt = X.y_bound(o, rb, roundings=5) + TANH_ULPS * 2 * U * rb.y.abs()
        ddz = o.dy.abs() * (2 * rb.y.abs() * dt + dt * dt + 2 * U) + U * rb.dz.abs()
    extra_g = (ddz * rb.xh.abs()).sum(dims) if tanh else 0.0
    extra_b = ddz.sum(dims) if tanh else 0.0
    ratio("dgamma", b["dgamma"], rb.dgamma, (P.run + 3) * U * (rb.dz * rb.xh).abs().sum(dims) + U * rb.dgamma.abs() + extra_g)
    ratio("dbeta", b["dbeta"], rb.dbeta, (P.run + 1) * U * rb.dz.abs().sum(dims) + U * rb.dbeta.abs() + extra_b)
    dxb = P.dx_bound(o, rb, True, roundings=7 if P.bf16 else 8, run=P.run, ddz=ddz) + half16 * rb.dx.abs()
    ratio("dx", b["dx"], rb.dx, dxb, P.owner)
    # worst error / bound per quantity (pytest -s; DESIGN §7b records them)
    print(f"bn-real {'cl' if P.bf16 else 'fp32'} {case.name} {mode}: " + " ".join(f"{k}={v:.3g}" for k, v in fig.items()))
    assert all(v <= 1.0 for v in fig.values()), fig


REAL_MODES = ("leaky", "dropout", "none")
REAL32 = [(c, REAL_MODES[i % 3]) for i, c in enumerate(X.CASES32)]
REAL_CL = [(c, REAL_MODES[i % 3]) for i, c in enumerate(X.CASES_CL)]


@pytest.mark.parametrize("case,mode", REAL32, ids=[f"{c.name}-{m}" for c, m in REAL32])
def test_bn_real_fp32(dev, case, mode):
    check_real_case(Path32(case), dev, mode)


@pytest.mark.parametrize("case,mode", REAL_CL, ids=[f"{c.name}-{m}" for c, m in REAL_CL])
def test_bn_real_cl(dev, case, mode):
    check_real_case(PathCL(case), dev, mode)


@pytest.mark.parametrize("name", X.TANH_CASES)
def test_bn_tanh_fp32(dev, name):
    """The Tanh branch of the apply and reduce kernels (small kernel and rows kernels): not exact, so real-valued input against fp64 within the rounding bound plus
    tanhf's documented error; the expected value is never taken from the device."""
    check_real_case(Path32(X.by_name(X.CASES32, name)), dev, "tanh")
