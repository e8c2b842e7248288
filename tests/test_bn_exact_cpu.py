"""Host only: the exact-integer BatchNorm suite's own construction (tests/exactbn.py), for every case of its tables —
  * the helper's fp64 reference equals F.batch_norm in fp64 plus autograd;
  * the quantities the GPU tests compare bit for bit really are fp32 values (a case that claims exactness it does not have fails here, not on the GPU);
  * the tests' copy of the dispatch arithmetic sends each case to the kernel variant it is meant to hit."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import exactbn as X

BIG = 2_000_000      # elements: beyond this the autograd comparison runs in one mode only (the formulas do not depend on the size)


def batch_norm(x, rm, rv, gamma, beta, training, momentum, eps):
    """F.batch_norm's operator without its argument check: F.batch_norm refuses eps = 0, which the kernels' C ABI accepts and the integer scheme needs"""
    return torch.batch_norm(x, gamma, beta, rm, rv, training, momentum, eps, False)


def autograd_reference(o, mode, eps, momentum=0.5):
    x, gamma, beta = (t.clone().requires_grad_(True) for t in (o.x, o.gamma, o.beta))
    C = x.shape[1]
    use_mask, act = X.act_of(mode)
    if mode == "eval":
        rm, rv = o.rm.clone(), o.rv.clone()
        h = batch_norm(x, rm, rv, gamma, beta, False, momentum, eps)
    else:
        rm, rv = torch.zeros(C, dtype=torch.float64), torch.ones(C, dtype=torch.float64)
        h = batch_norm(x, rm, rv, gamma, beta, True, momentum, eps)
    if use_mask:
        h = h * o.mask.view(o.mask.shape + (1,) * (x.dim() - 2))
    y = F.leaky_relu(h, X.SLOPE) if act == "leaky" else torch.tanh(h) if act == "tanh" else h
    dx, dg, db = torch.autograd.grad((y * o.dy).sum(), [x, gamma, beta])
    return y.detach(), dx, dg, db, rm, rv


def close(a, b, tol=1e-11):
    return float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


def modes_for(case):
    return X.MODES if math.prod(case.shape) < BIG else ("dropout",)


@pytest.mark.parametrize("case", X.CASES32 + X.CASES_CL, ids=lambda c: c.name)
def test_reference_is_batch_norm_with_autograd(case):
    o = X.exact_operands(case.name, case.shape)
    for mode in modes_for(case):
        r = X.reference(o, mode)
        y, dx, dg, db, rm, rv = autograd_reference(o, mode, 0.0)
        assert close(r.y, y) and close(r.dx, dx) and close(r.dgamma, dg) and close(r.dbeta, db), (case.name, mode)
        if mode != "eval":
            assert close(r.rm, rm) and close(r.rv, rv)
    if math.prod(case.shape) < BIG:      # ... and with real-valued operands, eps and the Tanh branch
        oo = X.real_operands(case.name, case.shape)
        for mode in ("dropout", "tanh"):
            r = X.reference(oo, mode, eps=1e-5, momentum=0.1, slope=0.2 if mode != "tanh" else 0.0, rm0=torch.zeros_like(oo.rm), rv0=torch.ones_like(oo.rv))
            x, gamma, beta = (t.clone().requires_grad_(True) for t in (oo.x, oo.gamma, oo.beta))
            rm, rv = torch.zeros_like(oo.rm), torch.ones_like(oo.rv)
            h = F.batch_norm(x, rm, rv, gamma, beta, True, 0.1, 1e-5)
            if mode == "dropout":
                h = h * oo.mask.view(oo.mask.shape + (1,) * (x.dim() - 2))
            y = F.leaky_relu(h, 0.2) if mode == "dropout" else torch.tanh(h)
            dx, dg, db = torch.autograd.grad((y * oo.dy).sum(), [x, gamma, beta])
            assert close(r.y, y.detach(), 1e-10) and close(r.dx, dx, 1e-9) and close(r.dgamma, dg, 1e-9) and close(r.dbeta, db, 1e-9), (case.name, mode)
            assert close(r.rm, rm) and close(r.rv, rv)


@pytest.mark.parametrize("case", X.CASES32, ids=lambda c: c.name)
def test_exactness_claims_fp32(case):
    o = X.exact_operands(case.name, case.shape)
    count = math.prod(case.shape) // case.shape[1]
    assert float(o.x.abs().max()) <= 12 and float(o.m.abs().max()) <= 8 and set(o.a.tolist()) <= {1.0, 2.0, 4.0}
    for mode in modes_for(case):
        r = X.reference(o, mode)                                            # the forward pass: the batch's own statistics
        rb = X.reference(o, mode, mean=o.m, invstd=1.0 / o.a) if mode != "eval" else r      # the backward pass is handed m and 1 / a
        assert X.sums_exact(o, rb, X.RUN32, mode)
        assert bool((r.s0 == o.m * count).all()) == (count % 2 == 0)        # the +- balance holds iff the count is even ...
        if mode != "eval":
            assert X.stats_exact(o, r) == (count % 2 == 0)
        if count % 2 == 0 or mode == "eval":                                # ... and then everything the forward pass writes is an fp32 value
            assert bool(X.is_f32(r.mean).all()) and bool(X.is_f32(r.invstd).all()) and bool(X.y_exact(o, r).all())
            assert mode == "eval" or bool(X.is_f32(r.rm).all())
        assert bool(X.y_exact(o, rb).all())
        assert bool(X.is_f32(rb.dgamma).all()) and bool(X.is_f32(rb.dbeta).all())
        ex = X.dx_exact(o, rb)
        if count & (count - 1) == 0 or mode == "eval":                      # a power-of-two count: dx is exact everywhere
            assert bool(ex.all()), (case.name, mode, float(ex.double().mean()))
        assert bool((rb.dx[~ex & (X.dx_bound(o, rb) == 0)] == 0).all())      # a zero bound without the claim: only where every summand is zero


@pytest.mark.parametrize("case", X.CASES_CL, ids=lambda c: c.name)
def test_exactness_claims_cl(case):
    o = X.exact_operands(case.name, case.shape)
    count = math.prod(case.shape) // case.shape[1]
    assert float(o.x.abs().max()) <= 16 and bool(X.is_bf16(o.x).all()) and bool(X.is_bf16(o.dy).all())
    for mode in X.MODES:
        r = X.reference(o, mode)
        rb = X.reference(o, mode, mean=o.m, invstd=1.0 / o.a) if mode != "eval" else r
        assert X.sums_exact(o, rb, X.RUN_CL, mode)
        assert bool(X.is_bf16(rb.y).all())
        if count % 2 == 0 or mode == "eval":
            assert bool(X.y_exact(o, r).all()) and bool(X.is_bf16(r.y).all())
        assert bool(X.is_f32(rb.dgamma).all()) and bool(X.is_f32(rb.dbeta).all())
        ex = X.cl_dx_exact(o, rb, mode != "eval")
        if case.want.get("count_pow2") or mode == "eval":
            assert count & (count - 1) == 0 or mode == "eval"
            assert bool(ex.all()), (case.name, mode)
        assert bool((rb.dx[~ex & (X.cl_dx_bound(o, rb, training=mode != "eval") == 0)] == 0).all())      # as above
        assert float(rb.dx.abs().max()) <= 256


@pytest.mark.parametrize("case", X.CASES32, ids=lambda c: c.name)
def test_dispatch_prediction_fp32(case):
    d = X.dispatch32(case.shape, (case.layout,))
    N, C, D, H, W = X.five(case.shape)
    w = dict(case.want)
    assert d.kind == w.pop("kind"), d
    for key in ("split", "per_chan", "gpr", "inner", "groups"):
        if key in w:
            assert getattr(d, key) == w.pop(key), (key, d)
    if "rps" in w:
        assert d.rps == w.pop("rps")
    if w.pop("ragged_slot", False):
        assert d.per_chan % 1024 != 0
    if "empty_blocks" in w:
        assert sum(1 for s in range(d.split) if s * d.rps >= N * D) == w.pop("empty_blocks")
    if w.pop("seg_spans_rows", False):
        assert d.seg > d.gpr * D      # a block's segment runs over more than one sample's (n, d) rows: its decode crosses both boundaries
    if w.pop("clamped", False):
        assert d.seg * d.split > d.per_chan > d.seg * (d.split - 1)
    if w.pop("grid_stride", False):
        assert d.groups > 8192 * 256 and d.ew_blocks == 8192 and not d.rows
    assert not w, f"unchecked expectations {w}"
    if d.kind == "small":
        assert d.vec == 4 and C >= 32 and 64 <= d.per_chan <= 8192
    if d.kind == "rows":
        assert (H * W) % 1024 == 0 and not d.small
    # the same variant when y / dy / dx share the layout (the GPU tests give every operand the case's layout)
    assert X.dispatch32(case.shape, (case.layout,) * 3) == d


def test_dispatch_covers_every_branch():
    ds = [X.dispatch32(c.shape, (c.layout,)) for c in X.CASES32]
    assert {d.kind for d in ds} == {"small", "rows", "gen4", "gen1"}
    assert {d.ew for d in ds if not d.small} == {"ew_rows", "ew<4>", "ew<1>"}
    assert any(d.split > 1 for d in ds if d.kind == "gen4") and any(d.split > 1 for d in ds if d.kind == "gen1") and any(d.split > 1 for d in ds if d.kind == "rows")
    assert any(d.inner == 1 for d in ds)
    cl = [X.dispatch_cl(c.shape) for c in X.CASES_CL]
    assert {d.G for d in cl if d.combine == "xor"} >= {1, 2, 4, 8, 16, 32, 64} and {d.G for d in cl if d.combine == "serial"} >= {3, 5, 12, 24, 48, 96, 128}
    assert max(d.blocks for d in cl) == 1024


@pytest.mark.parametrize("case", X.CASES_CL, ids=lambda c: c.name)
def test_dispatch_prediction_cl(case):
    d = X.dispatch_cl(case.shape)
    w = dict(case.want)
    assert d.combine == w.pop("combine")
    for key in ("G", "blocks", "active", "per_thread"):
        if key in w:
            assert getattr(d, key) == w.pop(key), (key, d)
    if "lds_bytes" in w:
        assert 4 * case.shape[1] * 2 * 8 == w.pop("lds_bytes")      # the dynamic LDS both reduce launches ask for: 4 C 2 doubles
    if w.pop("idle_slots", False):
        assert d.P < d.pb
    w.pop("count_pow2", None)
    assert not w, f"unchecked expectations {w}"
    if d.combine == "xor":
        assert d.active == 256
    if case.name == "block_cap":
        assert d.P > 16384 and d.per_thread > 8 and d.per_thread % 4 != 0 and d.per_thread % 2 != 0


def test_layouts_are_what_they_say():
    for c in X.CASES32:
        t, storage = X.guarded(c.shape, c.layout, "cpu", body=7.0)
        assert t.shape == tuple(c.shape) and bool(torch.isnan(t).all() == False)
        before = storage.clone()
        t.fill_(1.0)
        assert X.untouched_outside(storage, before, c.shape, c.layout)
        assert bool(torch.isnan(storage[:X.GUARD]).all()) and bool(torch.isnan(storage[-X.GUARD:]).all())
    t, _ = X.guarded((2, 3, 5, 4, 4), "permuted", "cpu", body=0.0)
    assert t.permute(0, 2, 1, 3, 4).is_contiguous()
    t, _ = X.guarded((3, 5, 6, 8), "hw_transposed", "cpu", body=0.0)
    assert t.transpose(2, 3).is_contiguous()
    t, _ = X.guarded((4, 6, 8, 8), "misaligned", "cpu", body=0.0)
    assert t.is_contiguous() and t.storage_offset() % 4 == 1


def test_mismatch_report_names_the_owner():
    c = X.by_name(X.CASES32, "rows_empty_blocks")
    d = X.dispatch32(c.shape)
    want = torch.zeros(c.shape, dtype=torch.float64)
    got = want.clone().float()
    got[6, 4, 47, 63] = 3.0
    with pytest.raises(AssertionError) as e:
        X.assert_within("y", got, want, 0.0, c.shape, lambda i: X.owner32(d, c.shape, i))
    msg = str(e.value)
    assert "(6, 4, 0, 47, 63)" in msg and "difference 3.0" in msg and "row 6, block 27" in msg, msg
    ccl = X.by_name(X.CASES_CL, "serial_c24")
    dcl = X.dispatch_cl(ccl.shape)
    assert "slot" in X.owner_cl(dcl, ccl.shape, (1, 9, 0, 2, 3)) and "serial combine" in X.owner_cl(dcl, ccl.shape, (1, 9, 0, 2, 3))
    # bf16 results: between the roundings of the bound's ends, equal to the rounding of the reference where the bound is zero
    w = torch.tensor([[1.00390625, 3.0]], dtype=torch.float64)
    assert X.assert_within("t", w.bfloat16(), w, 0.0, (1, 2, 1, 1), bf16=True) == 0.0
    with pytest.raises(AssertionError):
        X.assert_within("t", torch.tensor([[1.0078125, 3.0]]).bfloat16(), w, 0.0, (1, 2, 1, 1), bf16=True)
