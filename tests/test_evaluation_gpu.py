"""GPU: the evaluation statistics' kernels against the numpy restatements of tests/test_evaluation_cpu.py.

Integer-valued inputs make every sum exact in fp64 whatever its order, so the fp64 MFMA's lane maps, the tails (rows no multiple of 4, columns no multiple of 16,
more than one 64 x 64 workgroup tile), the mirrored lower tiles, the diagonal mask and the table's gather are each held bit for bit; real-valued inputs are held to
summation bounds.  Measured worst values are printed (pytest -s) before each assertion."""
import numpy as np
import pytest

from tests import test_evaluation_cpu as R

pytestmark = pytest.mark.gpu
F32, F64, EPS = R.F32, R.F64, R.EPS


@pytest.fixture(scope="module")
def dev():
    import torch
    from dcvgan_amd import native
    native.lib()
    torch.cuda.set_device(0)
    return torch.device("cuda:0")


def to_dev(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def strided(a, pad, dev):
    """The rows of `a` as a row-strided device view, `pad` NaNs after every row."""
    import torch
    n, D = a.shape
    base = torch.full((n, D + pad), float("nan"), dtype=torch.float32).numpy()
    base[:, :D] = a
    return to_dev(base, dev)[:, :D]


# ---- moments ---------------------------------------------------------------------------------------------------------------------------------------------
MOMENT_SHAPES = [(1, 16), (4, 16), (7, 20), (5, 1), (37, 48), (130, 80), (64, 144), (9, 65)]      # (9, 65): one column past the 64-wide workgroup tile


@pytest.mark.parametrize("n,D", MOMENT_SHAPES)
def test_moments_integer_features_bit_for_bit(dev, n, D):
    from dcvgan_amd import evaluation as E
    x = np.random.default_rng(1000 * n + D).integers(-8, 9, size=(n, D)).astype(F32)
    fm = E.FeatureMoments(D, dev)
    l0 = E.launches()
    fm.update(to_dev(x, dev))
    assert E.launches() == l0 + 1 and fm.n == n
    xi = x.astype(np.int64)
    sd = fm.state_dict()
    assert np.array_equal(sd["sum"], xi.sum(0).astype(F64))
    assert np.array_equal(sd["gram"], (xi.T @ xi).astype(F64))


def test_moments_strided_rows_and_successive_updates(dev):
    from dcvgan_amd import evaluation as E, native
    x = np.random.default_rng(11).integers(-8, 9, size=(37, 48)).astype(F32)
    xi = x.astype(np.int64)
    want_s, want_g = xi.sum(0).astype(F64), (xi.T @ xi).astype(F64)
    a = E.FeatureMoments(48, dev).update(strided(x, 5, dev))      # row_stride 53 > D, NaN in the gap
    assert np.array_equal(a.state_dict()["sum"], want_s) and np.array_equal(a.state_dict()["gram"], want_g)
    b = E.FeatureMoments(48, dev)
    b.update(to_dev(x[:14], dev)).update(strided(x[14:], 3, dev))      # two calls: the second starts from the first's gram tiles
    assert b.n == 37 and np.array_equal(b.state_dict()["sum"], want_s) and np.array_equal(b.state_dict()["gram"], want_g)
    one = E.FeatureMoments(48, dev).update(to_dev(x, dev)[5:6])        # a single row of a larger tensor
    assert np.array_equal(one.state_dict()["gram"], np.outer(xi[5], xi[5]).astype(F64))
    for bad in (to_dev(x, dev).t(), to_dev(x.T, dev).t(), to_dev(x, dev)[:, ::2], to_dev(x, dev).double(), to_dev(x, dev)[:, :47], to_dev(x, dev).reshape(37, 6, 8)):
        with pytest.raises(native.NativeError):
            a.update(bad)
    assert a.n == 37
    nan = x.copy()
    nan[3, 7] = np.nan
    g = E.FeatureMoments(48, dev).update(to_dev(nan, dev)).state_dict()["gram"]
    assert np.isnan(g[7]).all() and np.isnan(g[:, 7]).all() and np.isfinite(np.delete(np.delete(g, 7, 0), 7, 1)).all()      # a non-finite feature propagates, and only there


def test_moments_real_features_within_the_summation_bound(dev):
    """fp32 Gaussian features with mean 3 (the covariance is a difference of large numbers).  Products of fp32 values are exact in fp64, so the kernel's and numpy's
    results are each within (n - 1) EPS of the true sum of |products|: |gram - ref| <= 4 n EPS (|X|^T |X|) elementwise."""
    from dcvgan_amd import evaluation as E
    n, D = 300, 48
    x = (np.random.default_rng(21).standard_normal((n, D)) + 3.0).astype(F32)
    xd = to_dev(x, dev)
    fm = E.FeatureMoments(D, dev).update(xd)
    s, g = fm.state_dict()["sum"], fm.state_dict()["gram"]
    ref_s, ref_g = R.gram_ref(x)
    bound_g, bound_s = 4 * n * EPS * (np.abs(x).astype(F64).T @ np.abs(x).astype(F64)), 4 * n * EPS * np.abs(x).astype(F64).sum(0)
    print(f"\n[moments] (300, 48): worst |gram - ref| / bound {np.max(np.abs(g - ref_g) / bound_g):.3g}, worst |sum - ref| / bound {np.max(np.abs(s - ref_s) / bound_s):.3g}")
    assert np.all(np.abs(g - ref_g) <= bound_g) and np.all(np.abs(s - ref_s) <= bound_s)
    assert np.array_equal(g, g.T)
    cov, ref_cov = fm.cov(), np.cov(x.astype(F64), rowvar=False)
    assert np.all(np.abs(cov - ref_cov) <= 2 * bound_g / (n - 1) + 1e-13)
    again = E.FeatureMoments(D, dev).update(xd)
    assert again.state_dict()["gram"].tobytes() == g.tobytes() and again.state_dict()["sum"].tobytes() == s.tobytes()      # the same calls, the same bits


def test_states_are_cleared_in_place(dev):
    """reset(): one launch of the library's copy, no new allocation; a NaN left in the state does not survive it."""
    from dcvgan_amd import evaluation as E
    x = np.random.default_rng(12).integers(-8, 9, size=(9, 65)).astype(F32)
    poisoned = x.copy()
    poisoned[2, 3] = np.nan
    fm = E.FeatureMoments(65, dev).update(to_dev(poisoned, dev))
    where, l0 = (fm.gram.data_ptr(), fm.sum.data_ptr()), E.launches()
    fm.reset()
    assert E.launches() == l0 + 1 and fm.n == 0 and (fm.gram.data_ptr(), fm.sum.data_ptr()) == where
    assert not fm._buf.cpu().numpy().any()
    fm.update(to_dev(x, dev))
    xi = x.astype(np.int64)
    assert np.array_equal(fm.state_dict()["gram"], (xi.T @ xi).astype(F64)) and np.array_equal(fm.state_dict()["sum"], xi.sum(0).astype(F64))
    z = _logits(5, 7)
    st = E.InceptionStats(7, dev).update(to_dev(np.full((5, 7), np.nan, dtype=F32), dev))
    assert np.isnan(st.state_host()).all()
    first = E.InceptionStats(7, dev).update(to_dev(z, dev)).state_host()
    st.reset().update(to_dev(z, dev))
    assert st.n == 5 and st.state_host().tobytes() == first.tobytes()


# ---- Inception sums --------------------------------------------------------------------------------------------------------------------------------------
def _logits(n, K):
    g = np.random.default_rng(31 * n + K)
    z = (g.standard_normal((n, K)) * 3.0).astype(F32)
    if n > 1:      # confident rows: logits of +-80
        z[1] = -80.0
        z[1, K // 2] = 80.0
        z[n - 1, 0] = 80.0
        z[n - 1, K - 1] = -80.0
    return z


@pytest.mark.parametrize("n,K", [(1, 2), (5, 7), (70, 400)])
def test_inception_sums_against_the_restatement(dev, n, K):
    """Every entry of the state is a sum of n (or n K) terms of one sign, each term a handful of correctly rounded operations and one exp / log whose two
    implementations differ by an ulp: relative 4 n K EPS per entry (1.3e-11 at the largest case)."""
    from dcvgan_amd import evaluation as E
    z = _logits(n, K)
    st = E.InceptionStats(K, dev)
    l0 = E.launches()
    st.update(to_dev(z, dev))
    assert E.launches() == l0 + 2 and st.n == n
    got, want = st.state_host(), R.inception_ref(z)
    rel = np.abs(got - want) / np.abs(want)
    bar = 4 * n * K * EPS
    print(f"\n[inception] ({n}, {K}): worst relative difference {rel.max():.3g}, bar {bar:.3g}; score {st.score():.6g}")
    assert np.all(np.isfinite(got)) and np.all(rel <= bar)
    want_score = E.inception_score_from_state(want, n)      # exp(A / n - H): its relative error is the absolute error of the exponent, <= bar (|A| / n + |H|) <= 2 bar log K
    assert abs(st.score() - want_score) <= 4 * bar * max(1.0, np.log(K)) * want_score
    st.update(strided(z, 3, dev))      # a second call, row-strided: the state doubles
    got2 = st.state_host()
    assert st.n == 2 * n and np.all(np.abs(got2 - 2 * want) <= 2 * bar * np.abs(want))


def test_inception_sums_of_equal_logits_are_exact(dev):
    from dcvgan_amd import evaluation as E
    n, K = 5, 8
    st = E.InceptionStats(K, dev).update(to_dev(np.full((n, K), -1.5, dtype=F32), dev))
    s = st.state_host()
    assert np.array_equal(s[:K], np.full(K, n / 8.0)) and abs(st.score() - 1.0) <= 1e-12


# ---- kernel distance -------------------------------------------------------------------------------------------------------------------------------------
def _tables(g, subsets, m, na, nb):
    """Explicit tables: distinct rows inside a subset; subset 1 (when there is one) shares its a rows with subset 0, reversed."""
    t = np.stack([np.stack([g.permutation(na)[:m], g.permutation(nb)[:m]]) for _ in range(subsets)]).astype(np.int32)
    if subsets > 1:
        t[1, 0] = t[0, 0][::-1]
    return t


@pytest.mark.parametrize("D", [16, 64])
@pytest.mark.parametrize("m", [2, 5, 33, 70])
@pytest.mark.parametrize("subsets", [1, 3])
def test_kid_sums_integer_features_bit_for_bit(dev, D, m, subsets):
    """Features in [-4, 4] and D a power of two: dot / D, + 1 and the cube are exact, and so is every sum.  m = 2 isolates the diagonal mask; m = 70 has two tiles per
    side (an off-diagonal tile of a symmetric block counts twice).  fa is row-strided: stride D + 5 takes the 4-byte loads, D + 4 the 16-byte ones."""
    from dcvgan_amd import evaluation as E
    g = np.random.default_rng(7 * D + 100 * m + subsets)
    na, nb = m + 9, m + 4
    fa, fb = g.integers(-4, 5, size=(na, D)).astype(F32), g.integers(-4, 5, size=(nb, D)).astype(F32)
    table = _tables(g, subsets, m, na, nb)
    want = R.kid_ref(fa, fb, table, exact=True)
    l0 = E.launches()
    for pad in (5, 4):
        got = E.kid_sums(strided(fa, pad, dev), to_dev(fb, dev), to_dev(table, dev)).cpu().numpy()
        assert got.shape == (subsets, 3) and np.array_equal(got, want), (pad, got, want)
    assert E.launches() == l0 + 4
    mean, std = E.kernel_distance(to_dev(fa, dev), to_dev(fb, dev), table=to_dev(table, dev))
    mmd2 = E.mmd2_from_sums(want, m)
    assert mean == float(mmd2.mean()) and std == float(mmd2.std())


def test_kid_sums_real_features_within_the_bound(dev):
    """Gaussian features, D = 20, m = 33.  A dot product of D exact products carries D EPS, the division, the + 1 and the two multiplications one rounding each
    (the cube triples the relative error of t): 3 (D + 2) EPS per k_ij; the sum of m^2 of them adds m^2 EPS: (3 (D + 2) + m^2) EPS sum |k_ij|."""
    from dcvgan_amd import evaluation as E, native
    g = np.random.default_rng(41)
    D, m, na, nb, subsets = 20, 33, 50, 41, 3
    fa, fb = g.standard_normal((na, D)).astype(F32), (g.standard_normal((nb, D)) * 1.3 + 0.2).astype(F32)
    table = _tables(g, subsets, m, na, nb)
    got = E.kid_sums(to_dev(fa, dev), to_dev(fb, dev), to_dev(table, dev)).cpu().numpy()
    want, scale = R.kid_ref(fa, fb, table), R.abs_kid_ref(fa, fb, table)
    bound = (3 * (D + 2) + m * m) * EPS * scale
    print(f"\n[kid] D 20 m 33: worst |sum - ref| / bound {np.max(np.abs(got - want) / bound):.3g}")
    assert np.all(np.abs(got - want) <= bound)
    assert E.kid_sums(to_dev(fa, dev), to_dev(fb, dev), to_dev(table, dev)).cpu().numpy().tobytes() == got.tobytes()
    bad = table.copy()
    bad[2, 1, 4] = nb                                    # a row outside fb
    with pytest.raises(ValueError):
        E.kernel_distance(to_dev(fa, dev), to_dev(fb, dev), table=to_dev(bad, dev))
    poisoned = E.kid_sums(to_dev(fa, dev), to_dev(fb, dev), to_dev(bad, dev)).cpu().numpy()      # the kernel does not follow it: NaN where it is used, nowhere else
    assert np.array_equal(poisoned[:2], got[:2]) and poisoned[2, 0] == got[2, 0] and np.isnan(poisoned[2, 1:]).all()
    with pytest.raises(native.NativeError):
        E.kid_sums(to_dev(fa, dev), to_dev(fb[:, :16], dev), to_dev(table, dev))


@pytest.mark.parametrize("na,nb,m,subsets,seed", [(5, 9, 5, 4, 0), (100, 34, 33, 3, 1), (1000, 4097, 70, 2, 2 ** 40 + 12345)])
def test_kid_draw_equals_the_mirror(dev, na, nb, m, subsets, seed):
    from dcvgan_amd import evaluation as E
    l0 = E.launches()
    t = E.kid_draw(na, nb, subsets, m, seed, dev)
    assert E.launches() == l0 + 1 and str(t.dtype) == "torch.int32" and tuple(t.shape) == (subsets, 2, m)
    assert np.array_equal(t.cpu().numpy(), E.draw_host(seed, subsets, m, na, nb))


def test_kernel_distance_with_drawn_subsets(dev):
    from dcvgan_amd import evaluation as E
    g = np.random.default_rng(51)
    fa, fb = g.standard_normal((40, 24)).astype(F32), (g.standard_normal((31, 24)) + 0.5).astype(F32)
    mean, std = E.kernel_distance(to_dev(fa, dev), to_dev(fb, dev), num_subsets=4, subset_size=16, seed=9)
    mmd2 = E.mmd2_from_sums(R.kid_ref(fa, fb, E.draw_host(9, 4, 16, 40, 31)), 16)
    assert abs(mean - mmd2.mean()) <= 1e-9 * abs(mmd2.mean()) and abs(std - mmd2.std()) <= 1e-9 * abs(mmd2.std())
    same, _ = E.kernel_distance(to_dev(fa, dev), to_dev(fa, dev), num_subsets=2, subset_size=1000, seed=0)      # m = min(subset_size, na, nb) = 40
    assert abs(same - E.mmd2_from_sums(R.kid_ref(fa, fa, E.draw_host(0, 2, 40, 40, 40)), 40).mean()) <= 1e-9


# ---- end to end ------------------------------------------------------------------------------------------------------------------------------------------
def test_evaluator_end_to_end(dev):
    """Generators of the smallest configuration the suite builds; 5 samples in batches of 2, so the last batch is truncated.  The extractor returns free views of
    the clip and records them; the reported numbers are those of numpy on the recorded features."""
    import torch
    from dcvgan_amd import evaluation as E, native, trainer
    from dcvgan_amd.configs import CONFIGS
    from dcvgan_amd.rng import PhiloxRng
    cfg = CONFIGS["isogd-depth"].scaled(batchsize=2, width_div=8)
    torch.manual_seed(cfg.seed)
    models = trainer.build_models(cfg, dev)
    r = PhiloxRng(123)
    for m in models.values():
        m._rng = r
    seen = []

    def extractor(xc, with_logits=True):
        flat = xc.permute(0, 2, 1, 3, 4).reshape(xc.shape[0], -1)
        feats, logits = flat[:, :24], flat[:, 24:31]
        seen.append((feats.cpu().numpy().copy(), logits.cpu().numpy().copy()))
        return feats, (logits if with_logits else None)

    ev = trainer.build_evaluator(cfg, models, extractor, kid_subsets=3, kid_subset_size=4, seed=5, max_features=16)
    assert ev.ggen is models["ggen"] and ev.cgen is models["cgen"]
    with pytest.raises(native.NativeError):
        ev.observe_real(torch.zeros(2, 3, 16, 64, 64))                 # a CPU clip
    g = torch.Generator().manual_seed(3)
    for _ in range(3):
        ev.observe_real((torch.rand(2, 3, 16, 64, 64, generator=g) * 2 - 1).to(dev))
    real = np.concatenate([f for f, _ in seen])
    assert ev.real.n == 6 and ev.n_real_feats == 6
    seen.clear()
    out = ev.evaluate(num_samples=5, batchsize=2)
    assert sorted(out) == ["fid", "is", "kid", "kid_std"] and all(isinstance(v, float) for v in out.values())
    assert len(seen) == 3 and ev.fake.n == 5 and ev.inception.n == 5 and ev.n_fake_feats == 5
    fake = np.concatenate([f for f, _ in seen])[:5]
    logits = np.concatenate([l for _, l in seen])[:5]
    assert np.array_equal(ev.fake_feats[:5].cpu().numpy(), fake) and np.array_equal(ev.real_feats[:6].cpu().numpy(), real)
    want_is = E.inception_score_from_state(R.inception_ref(logits), 5)
    want_fid = E.frechet_distance(R.moments_of(real.astype(F64)), R.moments_of(fake.astype(F64)))
    mmd2 = E.mmd2_from_sums(R.kid_ref(real, fake, E.draw_host(5, 3, 4, 6, 5)), 4)
    print(f"\n[evaluate] {out}; numpy: is {want_is!r}, fid {want_fid!r}, kid {mmd2.mean()!r} +- {mmd2.std()!r}")
    rel = lambda a, b: abs(a - b) <= 1e-9 * abs(b)
    assert rel(out["is"], want_is) and rel(out["fid"], want_fid) and rel(out["kid"], mmd2.mean()) and rel(out["kid_std"], mmd2.std())
    # a second evaluation clears the states of the first in place and uses them again
    states = (ev.fake, ev.inception, ev.fake.gram.data_ptr())
    seen.clear()
    out2 = ev.evaluate(num_samples=5, batchsize=2)
    assert (ev.fake, ev.inception, ev.fake.gram.data_ptr()) == states and ev.fake.n == 5 and ev.inception.n == 5
    fake2 = np.concatenate([f for f, _ in seen])[:5]
    assert not np.array_equal(fake2, fake)
    assert rel(out2["fid"], E.frechet_distance(R.moments_of(real.astype(F64)), R.moments_of(fake2.astype(F64))))
    assert rel(out2["is"], E.inception_score_from_state(R.inception_ref(np.concatenate([l for _, l in seen])[:5]), 5))
    # only what a metric needs is accumulated: no Gram without "fid"
    lean = trainer.build_evaluator(cfg, models, extractor, metrics=("is", "kid"), kid_subsets=2, kid_subset_size=4, max_features=8)
    lean.observe_real((torch.rand(4, 3, 16, 64, 64, generator=g) * 2 - 1).to(dev))
    assert sorted(lean.evaluate(num_samples=4, batchsize=2)) == ["is", "kid", "kid_std"] and lean.real is None and lean.fake is None
    # a metric whose inputs are missing is refused by name, before this module launches anything
    l0 = E.launches()
    blind = E.Evaluator(lambda xc: extractor(xc, with_logits=False), metrics=("is",))
    with pytest.raises(native.NativeError, match='"is"'):
        blind.evaluate(models["ggen"], models["cgen"], 5, 2)
    assert E.launches() == l0
    # the EMA twins are what an evaluator built with `ema` samples
    opts = trainer.build_optimizers(cfg, models)
    ema = trainer.build_ema(cfg, models, opts)
    ev2 = trainer.build_evaluator(cfg, models, extractor, ema=ema, metrics=("is",))
    assert ev2.ggen is ema.module("ggen") and ev2.cgen is ema.module("cgen")
    assert np.isfinite(ev2.evaluate(num_samples=2, batchsize=2)["is"])
