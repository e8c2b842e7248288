"""GPU: device-side spectral normalisation — dcv_spectral_update_multi / dcv_spectral_project_multi bit for bit on inputs whose arithmetic is exact in
any order, against an fp64 host evaluation with worst-case bounds, against torch.nn.utils.spectral_norm, convergence, the edge cases, and the feature through
ops.conv / layers.run / trainer.StepRunner.  Every case prints its figures (pytest -s).

THE BOUNDS (`_power_step`, `_projection`).  A sum of n fp32 products, formed in any order with any mix of fp32 and wider partial sums, is within n * 2^-23 * sum|terms| of the exact
sum (each product and each of at most n - 1 additions rounds once, relative 2^-24 each, first order; 2^-23 leaves the second order).  Everything else is carried
through the formulas to first order, times 1.001 for the dropped second-order terms (the relative errors are ~1e-5): a normalised vector x = y / |y| moves by at
most B_y / |y| + |x| |B_y|_2 / |y| plus 3 roundings of 2^-24 (the norm's reciprocal, its rounding to fp32, the product); sigma = u^T s by sum(|u| B_s + |s| B_u)
plus its own rounding; W / sigma by |W / sigma| (B_sigma / sigma + 4 * 2^-24); the projection (G - c u v^T) / sigma, c = <G, W / sigma>, by
(B_c |u v| + |c| (B_u |v| + |u| B_v) + 8 * 2^-24 (|G| + |c u v|)) / sigma + |P| B_sigma / sigma (c's, the product's, the fma's, the reciprocal's and the last
product's roundings are 6 of those 8)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import rig

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
EPS = 1e-12
U23, U24 = 2.0 ** -23, 2.0 ** -24
GUARD = 8      # elements of NaN on either side of every carved tensor
SN_KC, SN_MR, SN_EB, SN_MT = 256, 4, 4096, 24      # the kernels' chunk constants (csrc/elementwise.hip): columns per block, rows per block, elements per block, tensors per table


def update_launches(n, n_iter, guarded=False):
    """The header's formula."""
    return math.ceil(n / SN_MT) * (2 * n_iter + 1 if n_iter > 0 else 2) + (1 if guarded else 0)


def project_launches(n):
    return 2 * math.ceil(n / SN_MT)


# ---- raw calls -------------------------------------------------------------------------------------------------------------------------------------------
def _arr(ts):
    from dcvgan_amd.native import c_array
    return c_array(ts)


def _shape_arrays(ws):
    from dcvgan_amd.native import c_array
    return c_array([w.shape[0] for w in ws], C.c_int32), c_array([w.shape[1] for w in ws], C.c_int32)


def _workspace(ws):
    from dcvgan_amd.native import lib
    rows, cols = _shape_arrays(ws)
    need = lib().dcv_spectral_workspace_bytes(len(ws), rows, cols)
    assert need > 0
    return torch.empty(need, dtype=torch.uint8, device=DEV)


def _update(ws, wsn, us, vs, sgs, n_iter, state=None, scratch=None):
    from dcvgan_amd.native import check, lib, ptr, stream_ptr
    rows, cols = _shape_arrays(ws)
    scratch = scratch if scratch is not None else _workspace(ws)
    check(lib().dcv_spectral_update_multi(len(ws), _arr(ws), _arr(wsn), _arr(us), _arr(vs), _arr(sgs), rows, cols, n_iter, EPS, ptr(state), ptr(scratch), scratch.numel(),
                                          stream_ptr()), "dcv_spectral_update_multi")


def _project(gs, wsn, us, vs, sgs, scratch=None):
    from dcvgan_amd.native import check, lib, ptr, stream_ptr
    rows, cols = _shape_arrays(wsn)
    scratch = scratch if scratch is not None else _workspace(wsn)
    check(lib().dcv_spectral_project_multi(len(gs), _arr(gs), _arr(wsn), _arr(us), _arr(vs), _arr(sgs), rows, cols, EPS, ptr(scratch), scratch.numel(), stream_ptr()),
          "dcv_spectral_project_multi")


class _Arena:
    """Tensors carved out of ONE NaN-filled buffer with NaN bands between them; `odd` puts a tensor on an element offset that is 1 modulo 4 (4-byte alignment only)."""

    def __init__(self, total):
        self.host = torch.full((total,), float("nan"), dtype=torch.float32)
        self.pos, self.spans = GUARD, []

    def put(self, t, odd=False):
        n = t.numel()
        a = (self.pos + 3) // 4 * 4 + (1 if odd else 0)
        assert a + n + GUARD <= self.host.numel()
        self.host[a:a + n] = t.reshape(-1).float()
        self.spans.append((a, n, tuple(t.shape)))
        self.pos = a + n + GUARD
        return len(self.spans) - 1

    def upload(self):
        self.dev = self.host.to(DEV)
        assert self.dev.data_ptr() % 16 == 0
        return [self.dev[a:a + n].view(shape) for a, n, shape in self.spans]

    def bands_intact(self):
        mask = torch.ones(self.host.numel(), dtype=torch.bool)
        for a, n, _ in self.spans:
            mask[a:a + n] = False
        return bool(torch.isnan(self.dev.cpu()[mask]).all())


# ---- fp64 evaluation with bounds ---------------------------------------------------------------------------------------------------------------------------
def _normalised(y, By):
    nrm = max(float(y.norm()), EPS)
    x = y / nrm
    return x, 1.001 * (By / nrm + x.abs() * float(By.norm()) / nrm) + 3 * U24 * x.abs()


def _power_step(W, u, Bu, n_iter=1):
    """(u, v, s, sigma, W / sigma) in fp64 after n_iter power iterations from u, each with its bound."""
    M, K = W.shape
    A = W.abs()
    for _ in range(n_iter):
        t = W.t() @ u
        Bt = M * U23 * (A.t() @ u.abs()) + A.t() @ Bu
        v, Bv = _normalised(t, Bt)
        s = W @ v
        Bs = K * U23 * (A @ v.abs()) + A @ Bv
        u, Bu = _normalised(s, Bs)
    sigma = float(u @ s)
    Bsigma = 1.001 * float(u.abs() @ Bs + s.abs() @ Bu) + U23 * abs(sigma)
    se = max(sigma, EPS)
    Wsn = W / se
    BWsn = Wsn.abs() * (1.001 * Bsigma / se + 4 * U24)
    return dict(u=u, Bu=Bu, v=v, Bv=Bv, sigma=sigma, Bsigma=Bsigma, Wsn=Wsn, BWsn=BWsn)


def _projection(G, Wsn, u, v, sigma, BWsn=0.0, Bu=0.0, Bv=0.0, Bsigma=0.0):
    """(P, bound, c, B_c) of P = (G - c u v^T) / sigma in fp64; the B_* are the bounds of the inputs the device computed for itself (0: the device's own values)."""
    n = G.numel()
    c = float((G * Wsn).sum())
    Bc = n * U23 * float((G * Wsn).abs().sum()) + (float((G.abs() * BWsn).sum()) if torch.is_tensor(BWsn) else 0.0)
    se = max(sigma, EPS)
    uv = torch.outer(u, v)
    P = (G - c * uv) / se
    Buv = (torch.outer(Bu, v.abs()) + torch.outer(u.abs(), Bv)) if torch.is_tensor(Bu) else 0.0
    B = 1.001 * (Bc * uv.abs() + abs(c) * Buv) / se + 8 * U24 * (G.abs() + abs(c) * uv.abs()) / se + 1.001 * P.abs() * Bsigma / se
    return P, B, c, Bc


def _ratio(got, want, bound):
    """max |got - want| / bound over the elements (0 / 0 counts as 0)."""
    err = (got.double().cpu() - want).abs()
    bound = bound if torch.is_tensor(bound) else torch.full_like(err, float(bound))
    assert bool(((err == 0) | (bound > 0)).all()), "an element differs where the bound is zero"
    return float((err / bound.clamp_min(1e-300)).max())


# ---- 1. exact, bit for bit ------------------------------------------------------------------------------------------------------------------------------------
# (M, K0, extra columns); the issue's six, then each chunk constant C at C - 1 and C + 1: SN_KC along K (255 = 64 + 191; 257 = 256 + 1 is in the six), SN_MR along M
# (3 is in the six; 5), the 4096-element blocks (5 x 819 = 4095, 17 x 241 = 4097), and the 256-thread strides over M (255, 257)
EXACT_SHAPES = [(1, 16, 0), (7, 64, 5), (32, 256, 1), (3, 1024, 3), (256, 4096, 0), (1, 16384, 0),
                (5, 64, 191), (5, 256, 563), (17, 64, 177), (255, 256, 0), (257, 1024, 0)]
ODD = {1, 3, 6, 8, 10}      # shapes carved at 4-byte-only alignment (every tensor of theirs)


def _hadamard_rows(rows, K0):
    """Rows of the Sylvester Hadamard matrix of order K0: H[i, j] = (-1)^popcount(i & j)."""
    x = (np.asarray(rows, dtype=np.int64)[:, None] & np.arange(K0, dtype=np.int64)[None, :])
    par = np.zeros_like(x)
    while x.any():
        par ^= x & 1
        x >>= 1
    return torch.from_numpy(1.0 - 2.0 * par.astype(np.float64))


def _exact_case(i, M, K0, r, gen):
    k = int(round(math.log2(K0))) // 2
    assert 4 ** k == K0 and M <= K0 and M * (K0 + r) <= 2 ** 21
    rows = [(m * 37 + 5) % K0 for m in range(M)]
    assert len(set(rows)) == M
    j = (3 * i + 1) % M
    W = torch.cat([_hadamard_rows(rows, K0), torch.randint(-3, 4, (M, r), generator=gen).double()], dim=1)
    W[j, K0:] = 0.0
    u0 = torch.zeros(M, dtype=torch.float64); u0[j] = 1.0
    G = torch.randint(-2, 3, (M, K0 + r), generator=gen).double()
    want = dict(sigma=float(2 ** k), u=u0.clone(), v=W[j] / 2 ** k, Wsn=W / 2 ** k)
    want["P"] = (G - float((G * want["Wsn"]).sum()) * torch.outer(want["u"], want["v"])) / want["sigma"]
    assert torch.equal(want["P"].float().double(), want["P"]), "the expected projection is not an fp32 number"
    return W, u0, G, want


@pytest.fixture(scope="module")
def exact():
    gen = torch.Generator().manual_seed(7)
    cases = [_exact_case(i, *shape, gen) for i, shape in enumerate(EXACT_SHAPES)]
    total = sum(3 * W.numel() + W.shape[0] + W.shape[1] + 1 + 6 * (GUARD + 5) for W, _, _, _ in cases) + GUARD
    arena = _Arena(total)
    for i, (W, u0, G, _) in enumerate(cases):
        odd = i in ODD
        arena.put(W, odd); arena.put(torch.full_like(W, 77.0), odd); arena.put(u0, odd); arena.put(torch.full((W.shape[1],), 55.0), odd)
        arena.put(torch.full((1,), 33.0), odd); arena.put(G, odd)
    ts = arena.upload()
    return cases, arena, [ts[q::6] for q in range(6)]


def test_exact_bit_for_bit(exact):
    from dcvgan_amd import native
    native.lib()
    cases, arena, (ws, wsn, us, vs, sgs, gs) = exact
    n = len(cases)
    assert sum(1 for t in ws if t.data_ptr() % 16 == 4) == len(ODD) and all(t.data_ptr() % 4 == 0 for t in ws + gs + wsn)
    w_before = [w.clone() for w in ws]
    g_before = [g.clone() for g in gs]
    n0 = native.launch_count()
    _update(ws, wsn, us, vs, sgs, 1)
    assert native.launch_count() - n0 == update_launches(n, 1) == 3
    torch.cuda.synchronize()

    def check_update(tag):
        for i, (W, u0, G, want) in enumerate(cases):
            shape = EXACT_SHAPES[i]
            assert float(sgs[i]) == want["sigma"], (tag, shape, float(sgs[i]), want["sigma"])
            assert torch.equal(us[i].double().cpu(), want["u"]), (tag, shape, "u")
            assert torch.equal(vs[i].double().cpu(), want["v"]), (tag, shape, "v")
            assert torch.equal(wsn[i].double().cpu(), want["Wsn"]), (tag, shape, "W / sigma")
    check_update("n_iter = 1")
    first = [t.clone() for t in wsn + us + vs + sgs]
    n0 = native.launch_count()
    _update(ws, wsn, us, vs, sgs, 3)
    assert native.launch_count() - n0 == update_launches(n, 3) == 7
    torch.cuda.synchronize()
    check_update("n_iter = 3")
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(first, wsn + us + vs + sgs)), "n_iter = 3 moved a bit"
    n0 = native.launch_count()
    _update(ws, wsn, us, vs, sgs, 0)      # sigma of the stored u, v: the same bits again
    assert native.launch_count() - n0 == update_launches(n, 0) == 2
    torch.cuda.synchronize()
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(first, wsn + us + vs + sgs)), "n_iter = 0 moved a bit"
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(g_before, gs)), "the update wrote a gradient"
    n0 = native.launch_count()
    _project(gs, wsn, us, vs, sgs)
    assert native.launch_count() - n0 == project_launches(n) == 2
    torch.cuda.synchronize()
    for i, (W, u0, G, want) in enumerate(cases):
        assert torch.equal(gs[i].double().cpu(), want["P"]), (EXACT_SHAPES[i], "projection")
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(w_before, ws)), "a weight was written"
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(first, wsn + us + vs + sgs)), "the projection wrote W / sigma, u, v or sigma"
    assert arena.bands_intact(), "a NaN guard band was written"
    print(f"\n[spectral exact] {n} shapes in one table, {len(ODD)} of them on 4-byte-only alignment: sigma, u, v, W / sigma and the projection exact; launches 3 / 7 / 2 / 2")


# ---- 2. ragged Gaussian table ---------------------------------------------------------------------------------------------------------------------------------
RAGGED = [(3, 5), (7, 33), (32, 48), (32, 192), (128, 1024), (64, 4100), (1, 16), (1, 2048), (2, 16), (4, 16), (5, 17), (16, 16), (9, 255), (9, 257), (33, 127),
          (64, 64), (8, 512), (31, 333), (1, 4097), (6, 683), (257, 19), (12, 1000), (100, 41), (3, 1366), (64, 96), (17, 241), (2, 2049), (40, 103), (13, 13), (256, 64)]


def _ragged_case(odd=(2, 5, 9, 20, 29)):
    gen = torch.Generator().manual_seed(23)
    assert len(RAGGED) == 30 > SN_MT
    Ws = [(torch.randn(s, generator=gen) * 0.02).float() for s in RAGGED]
    u0s = [torch.nn.functional.normalize(torch.randn(s[0], generator=gen, dtype=torch.float64), dim=0).float() for s in RAGGED]
    Gs = [torch.randn(s, generator=gen).float() for s in RAGGED]
    arena = _Arena(sum(3 * W.numel() + sum(W.shape) + 1 + 6 * (GUARD + 5) for W in Ws) + GUARD)
    for i, (W, u0, G) in enumerate(zip(Ws, u0s, Gs)):
        o = i in odd
        arena.put(W, o); arena.put(torch.zeros_like(W), o); arena.put(u0, o); arena.put(torch.zeros(W.shape[1]), o); arena.put(torch.zeros(1), o); arena.put(G, o)
    ts = arena.upload()
    return Ws, u0s, Gs, arena, [ts[q::6] for q in range(6)]


def test_ragged_table_against_fp64():
    from dcvgan_amd import native
    native.lib()
    Ws, u0s, Gs, arena, (ws, wsn, us, vs, sgs, gs) = _ragged_case()
    n = len(Ws)
    n0 = native.launch_count()
    _update(ws, wsn, us, vs, sgs, 1)
    assert native.launch_count() - n0 == update_launches(n, 1) == 6
    n0 = native.launch_count()
    _project(gs, wsn, us, vs, sgs)
    assert native.launch_count() - n0 == project_launches(n) == 4
    torch.cuda.synchronize()
    worst = dict(u=0.0, v=0.0, sigma=0.0, Wsn=0.0, P=0.0)
    for i, (W, u0, G) in enumerate(zip(Ws, u0s, Gs)):
        r = _power_step(W.double(), u0.double(), torch.zeros(W.shape[0], dtype=torch.float64))
        P, BP, c, Bc = _projection(G.double(), r["Wsn"], r["u"], r["v"], r["sigma"], r["BWsn"], r["Bu"], r["Bv"], r["Bsigma"])
        got = dict(u=_ratio(us[i], r["u"], r["Bu"]), v=_ratio(vs[i], r["v"], r["Bv"]), sigma=abs(float(sgs[i]) - r["sigma"]) / r["Bsigma"],
                   Wsn=_ratio(wsn[i], r["Wsn"], r["BWsn"]), P=_ratio(gs[i], P, BP))
        for k_, v_ in got.items():
            worst[k_] = max(worst[k_], v_)
            assert v_ <= 1.0, (RAGGED[i], k_, v_)
    assert all(torch.equal(w.cpu(), W) for w, W in zip(ws, Ws)) and arena.bands_intact()
    print(f"\n[spectral ragged] 30 tensors, 2 tables: worst error / bound  u {worst['u']:.3f}  v {worst['v']:.3f}  sigma {worst['sigma']:.3f}  "
          f"W/sigma {worst['Wsn']:.3f}  projection {worst['P']:.3f}")


# ---- 3. against torch -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["conv2d", "conv3d"])
def test_against_torch_spectral_norm(kind):
    from dcvgan_amd import native
    native.lib()
    gen = torch.Generator().manual_seed(31)
    conv = torch.nn.Conv2d(6, 10, 4, 2, 1, bias=False) if kind == "conv2d" else torch.nn.Conv3d(5, 12, 4, stride=(1, 2, 2), padding=(0, 1, 1), bias=False)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=gen) * 0.02)
    W = conv.weight.detach().clone()
    M, K = W.shape[0], W[0].numel()
    u0 = torch.nn.functional.normalize(torch.randn(M, generator=gen, dtype=torch.float64), dim=0).float()
    G = torch.randn(W.shape, generator=gen).float()
    # torch's own, in fp64 on the host: the legacy hook form, its u set to ours, the hook called once by hand (training mode: one power iteration)
    ref = torch.nn.utils.spectral_norm(torch.nn.Conv2d(6, 10, 4, 2, 1, bias=False).double() if kind == "conv2d" else
                                       torch.nn.Conv3d(5, 12, 4, stride=(1, 2, 2), padding=(0, 1, 1), bias=False).double(), n_power_iterations=1, eps=EPS)
    with torch.no_grad():
        ref.weight_orig.copy_(W.double()); ref.weight_u.copy_(u0.double())
    ref.train()
    for hook in ref._forward_pre_hooks.values():
        hook(ref, None)
    (ref.weight * G.double()).sum().backward()
    # the device
    w, w_sn, u, v, sg, g = (t.to(DEV) for t in (W.reshape(M, K), torch.zeros(M, K), u0, torch.zeros(K), torch.zeros(1), G.reshape(M, K)))
    _update([w], [w_sn], [u], [v], [sg], 1)
    _project([g], [w_sn], [u], [v], [sg])
    torch.cuda.synchronize()
    r = _power_step(W.reshape(M, K).double(), u0.double(), torch.zeros(M, dtype=torch.float64))
    P, BP, _, _ = _projection(G.reshape(M, K).double(), r["Wsn"], r["u"], r["v"], r["sigma"], r["BWsn"], r["Bu"], r["Bv"], r["Bsigma"])
    # this file's fp64 evaluation IS torch's (to the last few bits of fp64): the bounds then apply to torch's values
    assert float((ref.weight.detach().reshape(M, K) - r["Wsn"]).abs().max()) < 1e-13 and float((ref.weight_orig.grad.reshape(M, K) - P).abs().max()) < 1e-10 * float(P.abs().max())
    ratios = dict(Wsn=_ratio(w_sn, ref.weight.detach().reshape(M, K), r["BWsn"]), u=_ratio(u, ref.weight_u.detach(), r["Bu"]), v=_ratio(v, ref.weight_v.detach(), r["Bv"]),
                  grad=_ratio(g, ref.weight_orig.grad.reshape(M, K), BP))
    print(f"\n[spectral vs torch, {kind}] {M} x {K}: error / bound {', '.join('%s %.3f' % kv for kv in ratios.items())}")
    assert all(x <= 1.0 for x in ratios.values()), ratios


# ---- 4. convergence -------------------------------------------------------------------------------------------------------------------------------------------
def test_convergence():
    from dcvgan_amd import native
    native.lib()
    gen = torch.Generator().manual_seed(41)
    M, K = 32, 48
    U, _ = torch.linalg.qr(torch.randn(M, M, generator=gen, dtype=torch.float64))
    V, _ = torch.linalg.qr(torch.randn(K, M, generator=gen, dtype=torch.float64))
    sv = torch.tensor([3.0, 1.0] + [0.5 ** i for i in range(1, M - 1)], dtype=torch.float64)
    W = ((U * sv) @ V.t()).float()
    u0 = torch.nn.functional.normalize(torch.randn(M, generator=gen, dtype=torch.float64), dim=0).float()
    w, w_sn, u, v, sg = (t.to(DEV) for t in (W, torch.zeros(M, K), u0, torch.zeros(K), torch.zeros(1)))
    n0 = native.launch_count()
    _update([w], [w_sn], [u], [v], [sg], 30)
    assert native.launch_count() - n0 == update_launches(1, 30) == 61
    torch.cuda.synchronize()
    bar = (M + K) * U23
    top = float(torch.linalg.svdvals(w_sn.double().cpu())[0])
    print(f"\n[spectral convergence] 30 iterations on diag(3, 1, 0.5, ...): sigma - 3 = {float(sg) - 3.0:+.2e}, top singular value of W / sigma - 1 = {top - 1.0:+.2e} (bar {bar:.2e})")
    assert abs(float(sg) - 3.0) <= bar and abs(top - 1.0) <= bar


# ---- 5. edge cases --------------------------------------------------------------------------------------------------------------------------------------------
def test_zero_matrix_gives_zeros():
    from dcvgan_amd import native
    native.lib()
    shapes = [(1, 16), (5, 33), (32, 256)]
    ws = [torch.zeros(s).to(DEV) for s in shapes]
    wsn = [torch.full(s, 9.0).to(DEV) for s in shapes]
    us = [torch.nn.functional.normalize(torch.ones(s[0]), dim=0).to(DEV) for s in shapes]
    vs, sgs = [torch.full((s[1],), 9.0).to(DEV) for s in shapes], [torch.full((1,), 9.0).to(DEV) for s in shapes]
    gs = [torch.ones(s).to(DEV) for s in shapes]
    for n_iter in (1, 2, 0):
        _update(ws, wsn, us, vs, sgs, n_iter)
        torch.cuda.synchronize()
        for t in wsn + us + vs + sgs:
            assert bool((t == 0).all()), (n_iter, t)
    _project(gs, wsn, us, vs, sgs)
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(g).all()) and bool((g == 1.0 / EPS).all()) for g in gs)      # (G - 0) / max(0, eps), finite in fp32


def test_guard_skip_leaves_every_bit_and_repeatable():
    from dcvgan_amd import native
    native.lib()
    runs = []
    for rep in range(2):
        Ws, u0s, Gs, arena, (ws, wsn, us, vs, sgs, gs) = _ragged_case()
        state = torch.zeros(8).to(DEV)
        _update(ws, wsn, us, vs, sgs, 2, state=state)      # not skipped
        _project(gs, wsn, us, vs, sgs)
        torch.cuda.synchronize()
        runs.append(arena.dev.clone())
        if rep == 0:
            skip = torch.tensor([1.0, 0, 0, 0, 0, 1.0, 0, 0]).to(DEV)      # DCV_GUARD_SKIPPED = 5
            before = arena.dev.clone()
            n0 = native.launch_count()
            _update(ws, wsn, us, vs, sgs, 1, state=skip)
            assert native.launch_count() - n0 == update_launches(len(ws), 1, guarded=True) == 7
            torch.cuda.synchronize()
            assert torch.equal(before.view(torch.int32), arena.dev.view(torch.int32)), "a skipped update wrote u, v, sigma or W / sigma"
            assert not torch.equal(arena.dev[arena.spans[1][0]:][:15], arena.host.to(DEV)[arena.spans[1][0]:][:15])      # (and the applied one had written)
    assert torch.equal(runs[0].view(torch.int32), runs[1].view(torch.int32)), "two runs on the same inputs differ"


# ---- 6. module plumbing ---------------------------------------------------------------------------------------------------------------------------------------
def _disc(kind, seed=3):
    from dcvgan_amd import discriminator as D
    from dcvgan_amd import util
    torch.manual_seed(seed)
    m = (D.VideoDiscriminator if kind == "video" else D.ImageDiscriminator)(1, 3, False, 0, 4)
    m.apply(util.init_weights)
    return m.to(DEV).train()


def _inputs(kind, gen):
    sp = (16, 64, 64) if kind == "video" else (64, 64)
    xg = (torch.rand(2, 1, *sp, generator=gen) * 2 - 1).to(DEV).requires_grad_(True)
    xc = (torch.rand(2, 3, *sp, generator=gen) * 2 - 1).to(DEV).requires_grad_(True)
    return xg, xc


@pytest.mark.parametrize("kind", ["video", "image"])
def test_module_plumbing(kind):
    import copy
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    from dcvgan_amd import layers, native, ops_cl, optim
    from dcvgan_amd.rng import PhiloxRng
    native.lib()
    model = _disc(kind)
    twin = copy.deepcopy(model)
    model._rng, twin._rng = PhiloxRng(1), PhiloxRng(1)
    sn = optim.spectral_norm(model, n_init=3, seed=2)
    assert len(sn.convs) == 5 and sn.convs[-1].weight.shape[0] == 1      # the logit head: M = 1
    with torch.no_grad():
        for c, t in zip(sn.convs, [m for m in twin.modules() if isinstance(m, (torch.nn.Conv2d, torch.nn.Conv3d))]):
            assert not optim.is_spectral(t)
            t.weight.copy_(c.__dict__["_dcv_spectral"].w_sn)
    gen = torch.Generator().manual_seed(5)
    xg, xc = _inputs(kind, gen)
    xg2, xc2 = (t.detach().clone().requires_grad_(True) for t in (xg, xc))
    y, y2 = model(xg, xc), twin(xg2, xc2)
    cot = torch.randn(y.shape, generator=gen).to(DEV)
    y.backward(cot); y2.backward(cot)
    torch.cuda.synchronize()
    assert torch.equal(y, y2) and torch.equal(xg.grad, xg2.grad) and torch.equal(xc.grad, xc2.grad), "logits or input gradients differ from the twin on W / sigma"
    pairs = list(zip(sn.convs, [m for m in twin.modules() if isinstance(m, (torch.nn.Conv2d, torch.nn.Conv3d))]))
    assert all(torch.equal(c.weight.grad, t.weight.grad) for c, t in pairs)      # before the projection: dL/d(W / sigma), the same kernels on the same bits
    ptrs = [c.weight.grad.data_ptr() for c in sn.convs]
    n0 = native.launch_count()
    sn.project()
    assert native.launch_count() - n0 == project_launches(5) == 2
    torch.cuda.synchronize()
    worst = 0.0
    for c, t in pairs:
        M, K = c.weight.shape[0], c.weight[0].numel()
        P, B, _, _ = _projection(t.weight.grad.double().cpu().reshape(M, K), c.__dict__["_dcv_spectral"].w_sn.double().cpu().reshape(M, K), c.weight_u.double().cpu(),
                                 c.weight_v.double().cpu(), float(c.weight_sigma))
        r = _ratio(c.weight.grad.reshape(M, K), P, B)
        worst = max(worst, r)
        assert r <= 1.0, (tuple(c.weight.shape), r)
    # a second backward adds in place, with the library's kernels only
    y = model(xg.detach(), xc.detach())      # (inputs without a gradient: autograd's own sum into an existing input gradient is not what is looked at)
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        y.backward(cot)
        torch.cuda.synchronize()
    assert [c.weight.grad.data_ptr() for c in sn.convs] == ptrs
    kernels = {e.key: e.count for e in prof.key_averages() if e.device_type == DeviceType.CUDA}
    foreign = {k[:160]: n for k, n in kernels.items() if "at::" in k or "torch" in k.lower()}
    assert kernels and not foreign, foreign
    print(f"\n[spectral plumbing, {kind}] logits and input gradients bit-identical to the twin; projection error / bound {worst:.3f}; second backward: {sum(kernels.values())} launches, none foreign")
    # a stale W / sigma is refused, and renewed by update()
    with torch.no_grad():
        sn.convs[1].weight.mul_(1.0)      # (any in-place change bumps the version)
    with pytest.raises(native.NativeError, match=r"update\(\).*refresh\(\)"):
        model(xg, xc)
    sn.refresh()
    assert torch.equal(model(xg, xc).detach(), y.detach())
    # update() between a forward and its backward is refused
    y = model(xg, xc)
    sn.update()
    with pytest.raises(native.NativeError, match="rewritten after this forward"):
        y.backward(cot)
    # the 16-bit channels-last path is refused
    ops_cl.enable(True)
    try:
        with pytest.raises(native.NativeError, match="fp32-path only"):      # (the stem alone: at this width the 16-bit concat buffer would refuse first)
            layers.run(model.conv_g, ops_cl.from_f32(xg.detach()), model._rng)
    finally:
        ops_cl.enable(False)


# ---- 7. the iteration -----------------------------------------------------------------------------------------------------------------------------------------
def _runner(marked, seed=21, spectral_kw=True):
    from dcvgan_amd import native, trainer
    native.lib()
    cfg = rig.small_cfg()
    models, _ = rig.seeded_models(cfg, DEV, seed, 9)
    opts = trainer.build_optimizers(cfg, models, guard=dict(max_norm=10.0))
    sn = trainer.build_spectral_norm(cfg, models, opts, seed=4) if marked else None
    kw = dict(spectral=sn) if spectral_kw else {}
    return cfg, models, opts, sn, trainer.StepRunner(cfg, models, opts, trainer.build_loss(cfg), sync_losses=False, **kw)


def _data(cfg):
    return rig.clip_pair(cfg, DEV, 4)


_counted_steps = rig.counted_steps


def test_iteration():
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    from dcvgan_amd import native, trainer
    from dcvgan_amd.rng import PhiloxRng
    cfg, models, opts, sn, runner = _runner(True)
    xc, xg = _data(cfg)
    assert len(sn.convs) == 14 and sn.guard is opts["idis"].guard
    runner.step(xc, xg, 2)      # warm-up: optimiser state, workspaces and pointer tables are made here
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        (c2,), (o2,) = _counted_steps(runner, xc, xg, [3])
        torch.cuda.synchronize()
        u_before = [c.weight_u.cpu().double() for c in sn.convs]
        (c3,), (o3,) = _counted_steps(runner, xc, xg, [4])
        torch.cuda.synchronize()
    kernels = {e.key: e.count for e in prof.key_averages() if e.device_type == DeviceType.CUDA}
    foreign = {k[:160]: n for k, n in kernels.items() if "at::" in k or "torch" in k.lower()}
    assert not foreign, foreign
    mine = {k[:40]: n for k, n in kernels.items() if "sn_" in k}
    assert all(any(name in k for k in kernels) for name in ("sn_prepare", "sn_cols", "sn_rows", "sn_scale", "sn_inner", "sn_project")), sorted(kernels)[:60]
    for o in (o2, o3):
        assert all(math.isfinite(float(v)) for v in o.values()), o
        assert float(o["skipped_dis"]) == 0.0
    # launches: the unmarked run (the same guard) plus the documented constant, 14 convolutions in one table
    cfg_p, _, _, _, plain = _runner(False)
    plain.step(xc, xg, 2)
    (p2, p3), _ = _counted_steps(plain, xc, xg, [3, 4])
    extra = project_launches(14) + update_launches(14, 1, guarded=True)
    print(f"\n[spectral iteration] launches per iteration {c2}, {c3} vs unmarked {p2}, {p3}: + {extra} (projection 2, update 3 + 1 prepare); kernels {mine}")
    assert extra == 6 and c2 == p2 + extra and c3 == p3 + extra
    # spectral=None, and a StepRunner that was never given the argument: the same count
    _, _, _, _, bare = _runner(False, spectral_kw=False)
    bare.step(xc, xg, 2)
    (b2, b3), _ = _counted_steps(bare, xc, xg, [3, 4])
    assert (b2, b3) == (p2, p3)
    # u, sigma, W / sigma after the last iteration: ONE fp64 power step of (the weights after it, u before it)
    worst = dict(u=0.0, sigma=0.0, Wsn=0.0)
    for c, u0 in zip(sn.convs, u_before):
        M, K = c.weight.shape[0], c.weight[0].numel()
        r = _power_step(c.weight.detach().double().cpu().reshape(M, K), u0, torch.zeros(M, dtype=torch.float64))
        worst["u"] = max(worst["u"], _ratio(c.weight_u, r["u"], r["Bu"]))
        worst["sigma"] = max(worst["sigma"], abs(float(c.weight_sigma) - r["sigma"]) / r["Bsigma"])
        worst["Wsn"] = max(worst["Wsn"], _ratio(c.__dict__["_dcv_spectral"].w_sn.reshape(M, K), r["Wsn"], r["BWsn"]))
        assert c.__dict__["_dcv_spectral"].version == c.weight._version
    print(f"[spectral iteration] after the last iteration vs one fp64 power step: error / bound u {worst['u']:.3f}, sigma {worst['sigma']:.3f}, W/sigma {worst['Wsn']:.3f}")
    assert all(v <= 1.0 for v in worst.values()), worst
    # checkpoint round trip + refresh(): bit-identical logits
    sd = {n: {k: v.detach().cpu().clone() for k, v in models[n].state_dict().items()} for n in ("idis", "vdis", "gdis")}
    torch.manual_seed(99)
    fresh = trainer.build_models(cfg, DEV)
    sn2 = trainer.build_spectral_norm(cfg, fresh, trainer.build_optimizers(cfg, fresh), seed=77, n_init=1)
    for n in sd:
        fresh[n].load_state_dict(sd[n])
    with pytest.raises(native.NativeError):
        fresh["idis"](xg[:, :, 0], xc[:, :, 0])      # loaded, not refreshed: stale
    sn2.refresh()
    for n in sd:
        models[n]._rng, fresh[n]._rng = PhiloxRng(123), PhiloxRng(123)
        with torch.no_grad():
            a = models[n](xg[:, :, 0], xc[:, :, 0]) if n == "idis" else models[n](xg, xc)
            b = fresh[n](xg[:, :, 0], xc[:, :, 0]) if n == "idis" else fresh[n](xg, xc)
        assert torch.equal(a, b), n
    assert all(torch.equal(a.__dict__["_dcv_spectral"].w_sn, b.__dict__["_dcv_spectral"].w_sn) and torch.equal(a.weight_sigma, b.weight_sigma)
               for a, b in zip(sn.convs, sn2.convs))
