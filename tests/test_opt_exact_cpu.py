"""CPU: the host mirrors of tests/exactopt.py are themselves right — fmaf32 against exact rational arithmetic, adam_update against torch.optim.Adam and against an
fp64 evaluation with a counted error bound, guard_partials against integer sums, the table mirror against the covering property, and the guard's workspace size
against the blocks the kernel writes.  tests/test_opt_exact_gpu.py then holds the kernels to these mirrors bit for bit."""
import ctypes
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import exactopt as E

F32, F64, U32 = np.float32, np.float64, np.uint32
U = 2.0 ** -24
HP = dict(lr=2e-4, betas=(0.5, 0.999), eps=1e-8, weight_decay=1e-5)      # the reference's wiring


# ------------------------------------------------------------------------------------------------------------------------------------------------------
# fmaf32
# ------------------------------------------------------------------------------------------------------------------------------------------------------
def _round_f32(x):
    """a Fraction rounded to the nearest fp32, ties to even, denormals kept, as a Python float (inf on overflow)"""
    if x == 0:
        return 0.0
    sign, m = (-1.0 if x < 0 else 1.0), abs(x)
    e = m.numerator.bit_length() - m.denominator.bit_length()
    if Fraction(2) ** e > m:
        e -= 1                                    # 2^e <= m < 2^(e + 1)
    quantum = Fraction(2) ** (max(e, -126) - 23)
    q = m / quantum
    n = q.numerator // q.denominator
    rem = q - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n & 1):
        n += 1
    r = n * quantum
    return sign * (float("inf") if r >= Fraction(2) ** 128 else float(r))


def _exact(a, b, c):
    return np.array([_round_f32(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))) for x, y, z in zip(a, b, c)], F64).astype(F32)


def _mismatches(got, want):
    got, want = np.asarray(got, F32), np.asarray(want, F32)
    return int(np.sum(np.where(want == 0, got != 0, got.view(U32) != want.view(U32))))      # (an exact zero's sign is not at issue)


def _random_triples(n, seed):
    r = np.random.default_rng(seed)
    f = lambda lo, hi: (r.uniform(1, 2, n) * r.choice([-1.0, 1.0], n) * 2.0 ** r.integers(lo, hi, n)).astype(F32)
    a, b = f(-40, 40), f(-40, 40)
    near = (a.astype(F64) * b.astype(F64) * r.uniform(-2, 2, n) * 2.0 ** r.integers(-30, 30, n)).astype(F32)      # c within 2^+-30 of the product: both matter
    c = np.where(r.random(n) < 0.7, near, f(-100, 100))
    return a, b, c


def _built_triples(n, seed):
    """Triples whose exact sum lies within 2^-60 |result| of an fp32 midpoint, on either side, so that a rounding to double lands ON the midpoint.
    Kind B (c large, near a binade: c = 2^E (1 + k 2^-23), k small, 0 included): a b = -+ 2^j (1 - 2^-46) from a = 1 + 2^-23, b = 1 - 2^-23, with 2^j half of
    c's ulp (or a quarter, for the finer grid below a power of two), times an odd number: c + a b = midpoint -+ 2^(j-46).
    Kind A (the product large): a b is a midpoint itself (an odd 25-bit significand, the product of a 13- and a 12-bit factor) and c = +- a tiny power of two."""
    r = np.random.default_rng(seed)
    half = n // 2
    # kind B
    E_ = r.integers(-60, 60, half)
    k = r.integers(0, 4, half)
    c = ((1.0 + k * 2.0 ** -23) * 2.0 ** E_) * r.choice([-1.0, 1.0], half)
    odd = 2 * r.integers(0, 3, half) + 1
    finer = (k == 0) & (r.random(half) < 0.5)                       # below a power of two the grid is half as wide
    j = E_ - 24 - finer
    toward = np.where(finer, -np.sign(c), r.choice([-1.0, 1.0], half))      # the finer grid exists only towards zero
    a = ((1.0 + 2.0 ** -23) * odd * 2.0 ** (j // 2)) * toward
    b = (1.0 - 2.0 ** -23) * 2.0 ** (j - j // 2)
    A, B, C = [a.astype(F32)], [b.astype(F32) * np.ones(half, F32)], [c.astype(F32)]
    # kind A
    m = n - half
    x, y = 2 * r.integers(2 ** 11, 2 ** 12, m) + 1, 2 * r.integers(2 ** 10, 2 ** 11, m) + 1      # odd, product in [2^24, 2^25): 25 bits, the last one set
    prod = x * y
    keep = (prod >= 2 ** 24) & (prod < 2 ** 25)
    x, y = np.where(keep, x, 4097), np.where(keep, y, 4097)                                        # 4097^2 = 2^24 + 2^13 + 1
    ea, eb = r.integers(-30, 30, m), r.integers(-30, 30, m)
    A.append((x * 2.0 ** ea).astype(F32)); B.append((y * 2.0 ** eb).astype(F32))
    C.append((r.choice([-1.0, 1.0], m) * 2.0 ** (ea + eb - 40 - r.integers(0, 30, m))).astype(F32))
    return np.concatenate(A), np.concatenate(B), np.concatenate(C)


def _denormal_triples(n, seed):
    """results below 2^-126: random ones, and kind B on the denormal grid (c = k 2^-149, a b = +- 2^-150 (1 - 2^-46))"""
    r = np.random.default_rng(seed)
    half = n // 2
    a = (r.uniform(1, 2, half) * r.choice([-1.0, 1.0], half) * 2.0 ** r.integers(-80, -66, half)).astype(F32)
    b = (r.uniform(1, 2, half) * 2.0 ** r.integers(-80, -66, half)).astype(F32)
    c = (r.integers(-2 ** 20, 2 ** 20, half) * 2.0 ** -149).astype(F32)
    m = n - half
    a2 = (((1.0 + 2.0 ** -23) * 2.0 ** -75) * r.choice([-1.0, 1.0], m)).astype(F32)
    b2 = np.full(m, (1.0 - 2.0 ** -23) * 2.0 ** -75, F32)
    c2 = (r.integers(1, 2 ** 22, m) * r.choice([-1.0, 1.0], m) * 2.0 ** -149).astype(F32)
    return np.concatenate([a, a2]), np.concatenate([b, b2]), np.concatenate([c, c2])


def test_fmaf32_random_triples_match_exact_arithmetic():
    a, b, c = _random_triples(20000, 1)
    want = _exact(a, b, c)
    assert np.isfinite(want).all() and len(np.unique(want)) > 19000
    assert _mismatches(E.fmaf32(a, b, c), want) == 0


def test_fmaf32_built_double_rounding_triples():
    a, b, c = _built_triples(6000, 2)
    want = _exact(a, b, c)
    assert _mismatches(E.fmaf32(a, b, c), want) == 0
    naive = _mismatches(E.fmaf32_naive(a, b, c), want)
    print(f"\n[fmaf32] built triples: {len(a)}; the double evaluation rounded twice on {naive} of them, fmaf32 on 0")
    assert naive >= len(a) // 4, naive      # about half of the ties fall the wrong way: the triples are hard


def test_fmaf32_denormal_results():
    a, b, c = _denormal_triples(4000, 3)
    want = _exact(a, b, c)
    assert (np.abs(want) < 2.0 ** -126).all() and np.count_nonzero(want) > 3900
    assert _mismatches(E.fmaf32(a, b, c), want) == 0
    assert _mismatches(E.fmaf32_naive(a, b, c), want) > 0


def test_fmaf32_special_values():
    inf, nan = F32(np.inf), F32(np.nan)
    assert E.fmaf32(inf, F32(2), F32(1)) == inf and np.isnan(E.fmaf32(inf, F32(0), F32(1))) and np.isnan(E.fmaf32(nan, F32(1), F32(1)))
    assert np.isnan(E.fmaf32(inf, F32(1), -inf)) and E.fmaf32(F32(3e38), F32(2), F32(0)) == inf
    assert E.fmaf32(F32(0), F32(0), F32(5)) == F32(5) and E.fmaf32(F32(1), F32(1), F32(-1)) == 0


# ------------------------------------------------------------------------------------------------------------------------------------------------------
# adam_update
# ------------------------------------------------------------------------------------------------------------------------------------------------------
def _adam_run(n, steps, seed):
    p, g0, m, v = E.adam_case([n], seed, False)
    rng = np.random.default_rng(seed + 1)
    gs = [E.unique_normal(rng, n, 10.0 ** -(t % 3)) for t in range(steps)]
    return p, gs, m, v


def test_adam_update_against_torch_cpu():
    """the 1e-6 max-relative bar of tests/test_adam_gpu.py, over 10 steps at the reference's hyper-parameters (bit for bit it does NOT hold: torch's CPU kernels fuse)"""
    n = 70001
    p, gs, m, v = _adam_run(n, 10, 5)
    tp = torch.nn.Parameter(torch.from_numpy(p.copy()))
    opt = torch.optim.Adam([tp], foreach=False, fused=False, **HP)
    rel = lambda a, b: float(np.abs(a.astype(F64) - b.astype(F64)).max() / np.abs(b.astype(F64)).max())
    worst = 0.0
    for t, g in enumerate(gs, 1):
        tp.grad = torch.from_numpy(g.copy())
        opt.step()
        p, m, v = E.adam_update(p, g, m, v, E.adam_scalars(HP["lr"], *HP["betas"], HP["eps"], HP["weight_decay"], t, 1.0))
        st = opt.state[tp]
        for mine, theirs in ((p, tp.detach().numpy()), (m, st["exp_avg"].numpy()), (v, st["exp_avg_sq"].numpy())):
            worst = max(worst, rel(mine, theirs))
            assert rel(mine, theirs) <= 1e-6, t
    print(f"\n[adam mirror] 10 steps, n = {n}: worst max-relative difference from torch.optim.Adam on the CPU {worst:.3g}")


@pytest.mark.parametrize("betas,wd,gscale", [((0.5, 0.999), 1e-5, 1.0), ((0.9, 0.999), 0.0, 1.0 / 3.0), ((0.0, 0.99), 1e-5, 0.125)], ids=["reference", "first_branch", "beta1_0"])
def test_adam_update_against_fp64_with_a_counted_bound(betas, wd, gscale):
    """The fp32 mirror against adam_update64 on the same fp32 inputs.  A first-order bound is carried per element next to the fp64 values; u = 2^-24, every fp32
    scalar and every fp32 operation contributes one u, hats are the fp64 values:
      g' = g gs + wd p         the scalar gs, the product and the sum on g gs; the scalar wd, the product and the sum on wd p:   dg = 3u (|g gs| + |wd p|) + wd dp
      m' = lerp(m, g', w1)     carried error (1 - w1) dm + w1 dg exactly (either branch is linear in m and g'); locally the difference d = g' - m (u |d|), the
                               weight (w1 rounded; branch 2 rounds 1 - w1 once more, taken into the max below) and its product (2u), and the last sum (u |m'|):
                                                                                       dm' = (1 - w1) dm + w1 dg + 3u max(w1, 1 - w1) |d| + u |m'|
      v' = b2 v + w2 g' g'     a sum of non-negative terms, so relative errors: (rv + 2u) on b2 v (scalar, product), (2 dg / |g'| + 3u) on w2 g' g' (scalar, two
                               products), the larger of the two plus u for the sum:    rv' = max(rv + 2u, 2 dg / |g'| + 3u) + u
      denom = sqrt(v') / bc2s + eps    half of rv', the square root, the scalar bc2s and the division (3u); adding the positive eps (its own rounding u <= what
                               is there) costs one more u:                             rd = rv' / 2 + 4u
      p' = p - ss (m' / denom) the quotient q: dm' / denom + |q| (rd + u); the scalar ss and the product: 2u |ss q|; the sum: u |p'|:
                                                                                       dp' = dp + ss (dm' / denom + |q| (rd + u)) + 2u |ss q| + u |p'|
    Second-order terms are covered by a factor 1 + 2^-10 on every bound."""
    n, steps = 20011, 10
    lr, eps = 1e-3, 1e-8
    p, gs, m, v = _adam_run(n, steps, 9)
    P, M, V = p.astype(F64), m.astype(F64), v.astype(F64)
    dp, dm, rv = np.zeros(n), np.zeros(n), np.zeros(n)
    slack = 1.0 + 2.0 ** -10
    b1, b2 = betas
    w1 = 1.0 - b1
    worst = [0.0, 0.0, 0.0]
    for t, g in enumerate(gs, 1):
        G = g.astype(F64)
        gp = G * gscale + wd * P
        dg = 3 * U * (np.abs(G * gscale) + np.abs(wd * P)) + wd * dp
        d = gp - M
        P2, M2, V2 = E.adam_update64(P, G, M, V, lr, b1, b2, eps, wd, t, gscale)
        dm = (1 - w1) * dm + w1 * dg + 3 * U * max(w1, 1 - w1) * np.abs(d) + U * np.abs(M2)
        rv = np.maximum(rv + 2 * U, 2 * dg / np.abs(gp) + 3 * U) + U
        rd = rv / 2 + 4 * U
        ss = lr / (1.0 - b1 ** t)
        denom = np.sqrt(V2) / np.sqrt(1.0 - b2 ** t) + eps
        q = M2 / denom
        dp = dp + ss * (dm / denom + np.abs(q) * (rd + U)) + 2 * U * np.abs(ss * q) + U * np.abs(P2)
        P, M, V = P2, M2, V2
        p, m, v = E.adam_update(p, g, m, v, E.adam_scalars(lr, b1, b2, eps, wd, t, gscale))
        for i, (mine, ref, bound) in enumerate(((p, P, dp), (m, M, dm), (v, V, rv * V))):
            err = np.abs(mine.astype(F64) - ref)
            worst[i] = max(worst[i], float((err / (bound * slack)).max()))
            assert (err <= bound * slack).all(), (t, "pmv"[i], int(np.argmax(err / bound)))
    print(f"\n[adam mirror vs fp64] 10 steps, n = {n}: worst error / bound p {worst[0]:.3f} m {worst[1]:.3f} v {worst[2]:.3f}; "
          f"final bounds in u: p {float((dp / np.abs(P)).max() / U):.1f} (relative, worst element) v {float(rv.max() / U):.1f}")
    assert max(worst) > 0.01      # the bound is of the error's order, not a blanket


def test_adam_update_takes_both_lerp_branches_and_differs_between_them():
    p, g, m, v = E.adam_case([4099], 3, True)
    k2 = E.adam_scalars(2e-4, 0.5, 0.999, 1e-8, 1e-5, 1, 1.0)
    k1 = k2._replace(w1=F32(np.nextafter(F32(0.5), F32(0))))
    assert not k2.w1 < F32(0.5) and k1.w1 < F32(0.5)
    # the two branches round differently: with the same weight 0.5 written either way the results differ in some words
    d = (g * k2.gscale + k2.wd * p) - m
    first, second = m + F32(0.5) * d, (g * k2.gscale + k2.wd * p) - d * (F32(1) - F32(0.5))
    assert np.any(first.view(U32) != second.view(U32))
    assert np.array_equal(E.adam_update(p, g, m, v, k2)[1].view(U32), second.view(U32))


# ------------------------------------------------------------------------------------------------------------------------------------------------------
# the table mirror
# ------------------------------------------------------------------------------------------------------------------------------------------------------
def _random_size_lists(count, seed):
    r = np.random.default_rng(seed)
    out = [list(v) for v in E.LISTS.values()]
    while len(out) < count:
        k = int(r.integers(1, 80))
        pick = r.choice([0, 1, 3, 255, 256, 4095, 4096, 4097, 8191, 8193, 12290, 20000], k, p=[.3, .15, .1, .05, .05, .05, .1, .05, .05, .04, .03, .03])
        out.append([int(x) for x in pick])
    out.append([5] * 24 + [0] * 24 + [0] * 24 + [7])      # two tables without blocks in a row
    return out


SIZE_LISTS = _random_size_lists(300, 17)


def test_every_element_has_exactly_one_owner():
    for sizes in SIZE_LISTS:
        owners = E.block_owner(sizes)
        assert [o[4] for o in owners] == list(range(E.total_blocks(sizes)))      # partial indices contiguous across tables, a skipped table included
        per_tensor = {}
        for k, slot, t, blk, idx in owners:
            assert t == k * E.MT + slot and sizes[t] > 0
            per_tensor.setdefault(t, []).append(blk)
        assert per_tensor == {t: list(range(E.mt_blocks(n))) for t, n in enumerate(sizes) if n}
    for n in sorted({n for s in SIZE_LISTS for n in s} | set(E.RAGGED)):
        for order in (E.STRIDED, E.QUAD):
            seen = np.zeros(n, np.int32)
            for blk in range(E.mt_blocks(n)):
                for tid in range(E.NT):
                    for trip, j in enumerate(E.elements_of(n, blk, tid, order)):
                        seen[j] += 1
                        assert E.owner_of(j, order) == (blk, tid, trip)
            assert (seen == 1).all(), (n, order)


def test_skipped_table_and_block0():
    tabs = E.tables(E.ZEROS["skipped_table"])
    assert [t.launched for t in tabs] == [True, False, True] and [t.block0 for t in tabs] == [0, 25, 25]
    assert tabs[0].blocks == 25 and tabs[2].first_block == [0, 3, 4, 5]
    assert "table 2 slot 0" in E.describe(E.ZEROS["skipped_table"], 48, 8192) and "partial 27" in E.describe(E.ZEROS["skipped_table"], 48, 8192)


def test_adam_grid_second_trip():
    assert E.adam_grid(8192 * 256) == (8192, 1) and E.adam_grid(8192 * 256 + 1) == (8192, 2) and E.adam_grid(257) == (2, 1)
    assert "trip 1" in E.describe_single(8192 * 256 + 1, 8192 * 256)


# ------------------------------------------------------------------------------------------------------------------------------------------------------
# guard mirrors
# ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_guard_partials_integer_sums_both_orders():
    for name, sizes in E.LISTS.items():
        x = E.guard_int_case(sizes, E.MT + len(sizes))
        gs = E.Arena(sizes).split(x)
        want = np.array([float((gs[t][blk * E.MT_BLOCK:(blk + 1) * E.MT_BLOCK].astype(F64) ** 2).sum()) for _, _, t, blk, _ in E.block_owner(sizes)])
        for aligned, order in ((True, E.QUAD), (False, E.QUAD), (False, E.STRIDED)):
            part, cnt = E.guard_partials(gs, aligned, order)
            assert np.array_equal(part, want) and not cnt.any(), (name, aligned, order)
        # one element more or less is seen by the fp32 norm
        st = E.guard_decide(want, np.zeros(len(want)), E.Rule(), [1, 0, 0, 0, 0, 0, 0, 0])
        less = want.copy(); less[-1] -= float(x[-1]) ** 2
        if less.sum() > 0:
            assert E.guard_decide(less, np.zeros(len(want)), E.Rule(), [1, 0, 0, 0, 0, 0, 0, 0])[E.GRAD_NORM] != st[E.GRAD_NORM], name


def test_guard_partials_real_values_do_not_depend_on_alignment_in_quad_order():
    rng = np.random.default_rng(4)
    sizes = E.RAGGED
    gs = E.Arena(sizes).split(E.unique_normal(rng, sum(sizes), 1.0))
    a, _ = E.guard_partials(gs, True)
    b, _ = E.guard_partials(gs, False, E.QUAD)
    c, _ = E.guard_partials(gs, False, E.STRIDED)
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    assert not np.array_equal(a.view(np.uint64), c.view(np.uint64))      # and the strided order does: what the kernel's MT_QUAD_ORDER is for
    ref = np.array([float((gs[t][blk * 4096:(blk + 1) * 4096].astype(F64) ** 2).sum()) for _, _, t, blk, _ in E.block_owner(sizes)])
    assert np.abs(a / ref - 1).max() < 16 * U


def test_guard_partials_counts_nonfinite():
    g = np.ones(4097, F32)
    g[4095], g[4096], g[7] = np.inf, -np.inf, np.array([0x7fc12345], U32).view(F32)[0]
    part, cnt = E.guard_partials([g])
    assert list(cnt) == [2, 1] and np.isnan(part[0]) and np.isinf(part[1])
    st = E.guard_decide(part, cnt, E.Rule(skip_nonfinite=1), [1024, 3, 0, 0, 0, 0, 2, 0])
    assert st[E.NONFINITE] == 3 and st[E.SKIPPED] == 1 and st[E.SKIPPED_TOTAL] == 3 and st[E.CLIP_COEF] == 1 and st[E.LOSS_SCALE] == 1024


def test_guard_decide_scaler_sequence():
    ok, bad = (np.array([4.0]), np.array([0])), (np.array([4.0]), np.array([1]))
    rule = E.Rule(dynamic=1, growth_interval=2, max_norm=1.0)
    st = np.array([1024, 0, 0, 0, 0, 0, 0, 0], F32)
    seen = []
    for part, cnt in (ok, ok, bad, ok, ok):
        st = E.guard_decide(part, cnt, rule, st)
        seen.append((float(st[E.LOSS_SCALE]), float(st[E.GROWTH_TRACKER]), float(st[E.SKIPPED])))
    assert seen == [(1024, 1, 0), (2048, 0, 0), (1024, 0, 1), (1024, 1, 0), (2048, 0, 0)]
    big = E.guard_decide(*ok, E.Rule(dynamic=1, growth_interval=1), [3e38, 0, 0, 0, 0, 0, 0, 0])
    assert big[E.LOSS_SCALE] == F32(3e38) and big[E.GROWTH_TRACKER] == 0      # a growth that would overflow is not taken
    assert st[E.GRAD_NORM] == F32(2.0 / 1024) and st[E.CLIP_COEF] == 1.0


def test_ema_mirror():
    assert E.ema_w(0, 0.999, True) == F32(0.9) and E.ema_w(0, 0.999, False) == F32(1.0 - 0.999) and E.ema_w(10 ** 6, 0.999, True) == F32(1.0 - 0.999)
    assert E.ema_update(F32(0), F32(1), E.ema_w(3, 0.999, True)) == E.ema_w(3, 0.999, True)
    assert E.ema_update(F32(1e8), F32(1), F32(1)) == 0      # s - e rounds first


# ------------------------------------------------------------------------------------------------------------------------------------------------------
# the workspace the library asks for covers the blocks the kernel writes
# ------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from dcvgan_amd import native
    if not os.path.exists(native.LIB_PATH):      # as tests/test_abi_cpu.py: build it where it is missing
        import __graft_entry__ as g
        g.build()
    return native.lib()


def test_guard_workspace_covers_the_blocks(lib):
    for sizes in SIZE_LISTS:
        got = lib.dcv_grad_guard_workspace_bytes(ctypes.c_int64(sum(sizes)), len(sizes))
        assert got >= 12 * E.total_blocks(sizes), (sizes, got)
        assert got >= 12 * max(o[4] + 1 for o in E.block_owner(sizes)) if E.total_blocks(sizes) else got > 0
