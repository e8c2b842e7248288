"""GPU: the k-nearest-neighbour manifold metrics' kernels against the numpy mirror `evaluation.manifold_host`.

Features that are small integers make every dot, norm and distance an exact integer in fp64, so radii, counts, minima and the four metrics must equal the mirror bit
for bit — including the exact ties d2 == rad2 these inputs contain, which hold the <=.  Real-valued features are held to a rounding bound for the radii and minima
and, their closest margin asserted first, to exact counts and metrics.  Measured worst values are printed (pytest -s) before each assertion."""
import numpy as np
import pytest

from tests import rig
from tests import test_manifold_cpu as R

pytestmark = pytest.mark.gpu
F32, F64 = R.F32, R.F64
EPS = float(np.finfo(F64).eps)
KEYS = ("precision", "recall", "density", "coverage")
INT_CASES = [(70, 65, 16, 3), (130, 97, 20, 5), (200, 150, 64, 3), (33, 40, 7, 5), (4, 4, 1, 3), (17, 2, 5, 1)]
REAL_CASES = INT_CASES[:3]


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


def shifted(a, dev):
    """The rows of `a` contiguous, but starting one float into an allocation: no 16-byte alignment, so the guarded 4-byte reads."""
    import torch
    n, D = a.shape
    flat = torch.full((n * D + 1,), float("nan"), dtype=torch.float32).numpy()
    flat[1:] = a.reshape(-1)
    return to_dev(flat, dev)[1:].view(n, D)


_CASES = {}


def integer_case(idx):
    """(a, b, k, mirror) of INT_CASES[idx], or for idx = "dup" the first shape with duplicated rows; computed once and shared."""
    from dcvgan_amd import evaluation as E
    if idx not in _CASES:
        if idx == "dup":
            na, nb, D, k = INT_CASES[0]
            a, b = R.integer_case(77, na, nb, D)
            a[10] = a[3]; a[64] = a[3]; a[69] = a[3]      # four copies of one real row, over two row tiles: radius 0 at k = 3
            b[7] = a[3]; b[64] = b[1]                      # a fake on top of them, and a duplicated fake
        else:
            na, nb, D, k = INT_CASES[idx]
            a, b = R.integer_case(idx, na, nb, D)
        _CASES[idx] = (a, b, k, E.manifold_host(a, b, k))
    return _CASES[idx]


def real_case(idx):
    from dcvgan_amd import evaluation as E
    key = ("real", idx)
    if key not in _CASES:
        na, nb, D, k = REAL_CASES[idx]
        g = np.random.default_rng(100 + idx)
        a = g.standard_normal((na, D)).astype(F32)
        b = (0.8 * g.standard_normal((nb, D)) + 0.3).astype(F32)
        _CASES[key] = (a, b, k, E.manifold_host(a, b, k))
    return _CASES[key]


def device_parts(a_d, b_d, k, col_splits=0):
    """rad2 of both sides and (count, dmin2) of both directions, as numpy."""
    from dcvgan_amd import evaluation as E
    ra, rb = E.knn_radii(a_d, k, col_splits), E.knn_radii(b_d, k, col_splits)
    c_ba, m_ba = E.manifold_counts(b_d, a_d, ra, col_splits)
    c_ab, m_ab = E.manifold_counts(a_d, b_d, rb, col_splits)
    return {key: t.cpu().numpy() for key, t in dict(rad2_a=ra, rad2_b=rb, count_ba=c_ba, dmin2_ba=m_ba, count_ab=c_ab, dmin2_ab=m_ab).items()}


def assert_same_bits(got, want, what):
    for key in got:
        assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), (what, key, np.flatnonzero(got[key] != want[key])[:8])


# ---- bit for bit on small-integer features ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", list(range(len(INT_CASES))) + ["dup"])
def test_integer_features_bit_for_bit(dev, idx):
    from dcvgan_amd import evaluation as E
    a, b, k, h = integer_case(idx)
    n_ties = R.ties(a, b, k)
    print(f"\n[manifold int] {a.shape} x {b.shape}, k {k}: {n_ties} exact ties d2 == rad2; mirror " + ", ".join(f"{key} {h[key]:.4f}" for key in KEYS))
    if min(a.shape[0], b.shape[0]) >= 33:
        assert n_ties >= 10                                     # the inputs do hold the <=
    vals = [h[key] for key in KEYS]
    assert not all(v == 0.0 for v in vals) and not all(v == 1.0 for v in vals)
    a_d, b_d = to_dev(a, dev), to_dev(b, dev)
    assert np.array_equal(E.row_norms(a_d).cpu().numpy(), (a.astype(F64) ** 2).sum(axis=1))
    got = device_parts(a_d, b_d, k)
    assert_same_bits(got, {key: h[key] for key in got}, idx)
    l0 = E.launches()
    m = E.manifold_metrics(a_d, b_d, k, k)
    assert E.launches() - l0 == E.manifold_launches(k, k) == 12
    assert sorted(m) == sorted(KEYS) and all(isinstance(v, float) for v in m.values())
    assert {key: m[key] for key in KEYS} == {key: h[key] for key in KEYS}, (m, vals)
    if idx == "dup":
        assert np.array_equal(got["rad2_a"][[3, 10, 64, 69]], np.zeros(4))      # a duplicate is a neighbour at distance 0: self is excluded by index, not by value
        assert got["dmin2_ba"][7] == 0.0 and got["count_ba"][7] >= 4


def test_two_ks_and_single_pairs(dev):
    """The defaults' shape of a call: precision / recall at one k, density / coverage at another; and each pair alone."""
    from dcvgan_amd import evaluation as E
    a, b, _, _ = integer_case(1)
    a_d, b_d = to_dev(a, dev), to_dev(b, dev)
    h3, h5 = E.manifold_host(a, b, 3), E.manifold_host(a, b, 5)
    want = dict(precision=h3["precision"], recall=h3["recall"], density=h5["density"], coverage=h5["coverage"])
    l0 = E.launches()
    assert E.manifold_metrics(a_d, b_d) == want
    assert E.launches() - l0 == E.manifold_launches() == 17
    l0 = E.launches()
    assert E.manifold_metrics(a_d, b_d, metrics=("pr",)) == {key: want[key] for key in ("precision", "recall")}
    assert E.launches() - l0 == 12
    l0 = E.launches()
    assert E.manifold_metrics(a_d, b_d, metrics=("dc",)) == {key: want[key] for key in ("density", "coverage")}
    assert E.launches() - l0 == 10
    c, m = E.manifold_counts(a_d, b_d, None)                 # no radii: zero counts, the minima alone
    assert not c.cpu().numpy().any() and np.array_equal(m.cpu().numpy(), h5["dmin2_ab"])
    with pytest.raises(ValueError):
        E.manifold_metrics(a_d, b_d, metrics=("pr", "kid"))
    from dcvgan_amd import native
    with pytest.raises(native.NativeError):
        E.manifold_metrics(a_d[:5], b_d, 3, 5)               # five reals have no fifth neighbour
    with pytest.raises(native.NativeError):
        E.knn_radii(a_d[:3], 3)


# ---- the column split ---------------------------------------------------------------------------------------------------------------------------------------
def test_column_split_gives_the_same_bits(dev):
    """The k smallest of a multiset, integer sums and minima do not depend on the order: every split gives the bits of every other — on real-valued features,
    where a different order of ARITHMETIC would show."""
    na, nb, D, k = INT_CASES[1]
    g = np.random.default_rng(9)
    a_d, b_d = to_dev(g.standard_normal((na, D)).astype(F32), dev), to_dev((0.8 * g.standard_normal((nb, D)) + 0.3).astype(F32), dev)
    base = device_parts(a_d, b_d, k, 0)
    for s in (1, 2, 3, 64):
        assert_same_bits(device_parts(a_d, b_d, k, s), base, f"col_splits {s}")
    a, b, k, h = integer_case(1)
    a_d, b_d = to_dev(a, dev), to_dev(b, dev)
    for s in (1, 2, 3, 64):
        got = device_parts(a_d, b_d, k, s)
        assert_same_bits(got, {key: h[key] for key in got}, f"col_splits {s} (integers)")


# ---- layout -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", [1, 3])
def test_strided_and_unaligned_rows_give_the_same_bits(dev, idx):
    """A row stride above D (a multiple of four: still 16-byte reads; odd: the guarded reads) and a base one float into an allocation give the contiguous bits.  The
    padding holds NaNs: nothing past a row's D values is read into a result."""
    from dcvgan_amd import evaluation as E
    na, nb, D, k = INT_CASES[idx]
    g = np.random.default_rng(20 + idx)
    a, b = g.standard_normal((na, D)).astype(F32), (0.8 * g.standard_normal((nb, D)) + 0.3).astype(F32)
    base = device_parts(to_dev(a, dev), to_dev(b, dev), k)
    for what, fa, fb in (("stride D + 4", strided(a, 4, dev), strided(b, 4, dev)), ("stride D + 3", strided(a, 3, dev), strided(b, 3, dev)),
                         ("mixed", strided(a, 8, dev), to_dev(b, dev)), ("base + one float", shifted(a, dev), shifted(b, dev))):
        assert_same_bits(device_parts(fa, fb, k), base, what)
        assert np.array_equal(E.row_norms(fa).cpu().numpy(), E.row_norms(to_dev(a, dev)).cpu().numpy())
    assert E.manifold_metrics(shifted(a, dev), strided(b, 3, dev), k, k) == E.manifold_metrics(to_dev(a, dev), to_dev(b, dev), k, k)


# ---- real features ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", range(len(REAL_CASES)))
def test_real_features_within_the_rounding_bound(dev, idx):
    """Reals Gaussian, fakes 0.8 g + 0.3.  rad2 and dmin2 within 4 D eps (|x|^2 + |y|^2) of the mirror (eps = 2^-52; the row's own norm with the largest norm of the
    other side: kernel and mirror each round a D-term dot product and two D-term norms, and differ in the order of the dot product alone).  Counts and the four
    metrics exactly equal, given that the mirror's closest margin min |d2 - rad2| / (|x|^2 + |y|^2) is at least 1e-9 — asserted first, so that a change of inputs
    cannot hide a flipped comparison behind a near tie.
    Measured on MI355X: see DESIGN §17."""
    from dcvgan_amd import evaluation as E
    a, b, k, h = real_case(idx)
    D = a.shape[1]
    n_a, n_b = E._norms_host(a.astype(F64)), E._norms_host(b.astype(F64))
    d_ba, d_ab = E.d2_host(b, a), E.d2_host(a, b)
    margins = (np.abs(d_ba - h["rad2_a"][None, :]) / (n_b[:, None] + n_a[None, :]), np.abs(d_ab - h["rad2_b"][None, :]) / (n_a[:, None] + n_b[None, :]),
               np.abs(h["dmin2_ab"] - h["rad2_a"]) / (n_a + n_b[d_ab.argmin(axis=1)]))
    margin = min(float(m.min()) for m in margins)
    print(f"\n[manifold real] {a.shape} x {b.shape}, k {k}: closest margin {margin:.2e}; mirror " + ", ".join(f"{key} {h[key]:.4f}" for key in KEYS))
    assert margin >= 1e-9
    a_d, b_d = to_dev(a, dev), to_dev(b, dev)
    got = device_parts(a_d, b_d, k)
    bars = dict(rad2_a=n_a + n_a.max(), rad2_b=n_b + n_b.max(), dmin2_ba=n_b + n_a.max(), dmin2_ab=n_a + n_b.max())
    worst = {key: float((np.abs(got[key] - h[key]) / bars[key]).max()) for key in bars}
    print(f"[manifold real] worst |device - mirror| / (|x|^2 + |y|^2): " + ", ".join(f"{key} {v:.2e}" for key, v in worst.items()) + f"; bar {4 * D * EPS:.2e}")
    for key in bars:
        assert np.all(np.abs(got[key] - h[key]) <= 4 * D * EPS * bars[key]), key
    assert np.array_equal(got["count_ba"], h["count_ba"]) and np.array_equal(got["count_ab"], h["count_ab"])
    m = E.manifold_metrics(a_d, b_d, k, k)
    assert {key: m[key] for key in KEYS} == {key: h[key] for key in KEYS}, (m, h)


# ---- non-finite ---------------------------------------------------------------------------------------------------------------------------------------------
def test_a_nan_feature_gives_nan_metrics_and_is_nobodys_neighbour(dev):
    from dcvgan_amd import evaluation as E
    a, b, k, _ = integer_case(0)
    a = a.copy()
    a[5, 3] = np.nan
    a_d, b_d = to_dev(a, dev), to_dev(b, dev)
    m = E.manifold_metrics(a_d, b_d, k, k)
    assert sorted(m) == sorted(KEYS) and all(np.isnan(v) for v in m.values())
    assert all(np.isnan(v) for v in E.manifold_metrics(b_d, a_d).values())      # the NaN on the other side
    keep = np.arange(a.shape[0]) != 5
    rad = E.knn_radii(a_d, k).cpu().numpy()
    assert np.array_equal(rad[keep], E.knn_radii_host(a[keep], k)) and rad[5] == np.inf      # the row is no candidate of the others and has none itself
    h = E.manifold_host(a, b, k)
    got = device_parts(a_d, b_d, k)
    assert_same_bits(got, {key: h[key] for key in got}, "nan")
    assert np.array_equal(got["dmin2_ba"], E.counts_host(b, a[keep], None)[1]) and got["dmin2_ab"][5] == np.inf and got["count_ab"][5] == 0


# ---- end to end -------------------------------------------------------------------------------------------------------------------------------------------
def test_evaluator_reports_the_four_metrics(dev):
    """Generators of the smallest configuration the suite builds; 8 real clips, 7 samples in batches of 2 (the last batch truncated).  The extractor returns free
    views of the clip; the four keys are manifold_metrics on the stored buffers."""
    import torch
    from dcvgan_amd import evaluation as E, native, trainer
    cfg = rig.small_cfg()
    models, _ = rig.seeded_models(cfg, dev, cfg.seed, 123)

    def extractor(xc):
        flat = xc.permute(0, 2, 1, 3, 4).reshape(xc.shape[0], -1)
        return flat[:, :24], None

    ev = trainer.build_evaluator(cfg, models, extractor, metrics=("kid", "pr", "dc"), kid_subsets=3, kid_subset_size=4, seed=5, max_features=16)
    assert (ev.pr_k, ev.dc_k) == (3, 5) and ev.real is None
    g = torch.Generator().manual_seed(3)
    for i in range(4):
        if i == 2:      # five reals: "pr" could run, "dc" (k = 5) could not — refused by name before anything launches
            l0, n0 = E.launches(), native.launch_count()
            with pytest.raises(native.NativeError, match='"dc"'):
                ev.evaluate(num_samples=7, batchsize=2)
            assert E.launches() == l0 and native.launch_count() == n0
        ev.observe_real((torch.rand(3 if i == 1 else 2, 3, 16, 64, 64, generator=g) * 2 - 1).to(dev))      # 2 + 3 + 2 + 2 = 9 real clips
    assert ev.n_real_feats == 9
    with pytest.raises(native.NativeError, match='"dc"'):
        ev.evaluate(num_samples=5, batchsize=2)                 # too few samples for the fifth neighbour
    l0 = E.launches()
    out = ev.evaluate(num_samples=7, batchsize=2)
    assert E.launches() - l0 == 4 + 3 + E.manifold_launches(3, 5)      # four stores, the kernel distance's draw and sums, the manifold metrics' 17
    assert sorted(out) == ["coverage", "density", "kid", "kid_std", "precision", "recall"] and all(isinstance(v, float) for v in out.values())
    assert ev.n_fake_feats == 7
    real, fake = ev.real_feats[:9], ev.fake_feats[:7]
    want = E.manifold_metrics(real, fake, 3, 5)
    print(f"\n[evaluate] {out}")
    assert {key: out[key] for key in KEYS} == want
    h3, h5 = E.manifold_host(real.cpu().numpy(), fake.cpu().numpy(), 3), E.manifold_host(real.cpu().numpy(), fake.cpu().numpy(), 5)
    print(f"[evaluate] mirror: precision {h3['precision']}, recall {h3['recall']}, density {h5['density']}, coverage {h5['coverage']}")
    assert all(0.0 <= out[key] <= 1.0 for key in ("precision", "recall", "coverage")) and 0.0 <= out["density"] <= 9 / 5
    # a second evaluation fills the same buffers
    ptrs = (ev.real_feats.data_ptr(), ev.fake_feats.data_ptr())
    first = fake.cpu().numpy().copy()
    out2 = ev.evaluate(num_samples=7, batchsize=2)
    assert (ev.real_feats.data_ptr(), ev.fake_feats.data_ptr()) == ptrs and ev.n_fake_feats == 7 and ev.n_real_feats == 9
    assert not np.array_equal(ev.fake_feats[:7].cpu().numpy(), first)
    assert {key: out2[key] for key in KEYS} == E.manifold_metrics(ev.real_feats[:9], ev.fake_feats[:7], 3, 5)
