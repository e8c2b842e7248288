"""GPU: PRD's kernels against the numpy mirror `evaluation.prd_host`.

Integer features make every dot and every sum of rows exact in fp64, so seeds, assignments, centroids and histograms must equal the mirror bit for bit — including the
exact ties between duplicated centroids, which hold "the lowest index".  Where the centroids are means (not integers) the device's dot products differ from numpy's in
their last bits: the test then asserts FIRST, on the mirror, that every row of every run and iteration has either a margin of 1e-9 (|x|^2 + cn) between its best score
and every other one, or an exact tie between centroids with integer coordinates.  Measured worst values are printed (pytest -s) before each assertion."""
import numpy as np
import pytest

from tests import rig
from tests import test_prd_cpu as R
from tests.test_manifold_gpu import shifted, strided, to_dev

pytestmark = pytest.mark.gpu
F32, F64 = R.F32, R.F64
EPS = 2.0 ** -52
SHAPES = [(70, 65, 16, 20, 3), (130, 97, 20, 64, 2), (200, 150, 64, 20, 10), (33, 40, 7, 1, 1), (4, 4, 1, 3, 1)]      # (na, nb, D, C, R)
GAUSS = [(70, 65, 16, 20, 10), (200, 150, 64, 20, 10)]
T = 8


@pytest.fixture(scope="module")
def dev():
    import torch
    from dcvgan_amd import native
    native.lib()
    torch.cuda.set_device(0)
    return torch.device("cuda:0")


_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def union(a, b):
    from dcvgan_amd import evaluation as E
    x = np.concatenate([a, b]).astype(F64)
    with np.errstate(all="ignore"):
        return x, E._norms_host(x)


def integer_case(idx):
    """Features and explicit centroids in [-3, 3]: per run centroid 0 is a feature row, centroid 1 its duplicate, every third one another feature row."""
    def make():
        na, nb, D, C, Rn = SHAPES[idx]
        g = np.random.default_rng(40 + idx)
        a, b = g.integers(-3, 4, size=(na, D)).astype(F32), g.integers(-3, 4, size=(nb, D)).astype(F32)
        x = np.concatenate([a, b]).astype(F64)
        cent = g.integers(-3, 4, size=(Rn, C, D)).astype(F64)
        for r in range(Rn):
            for c in range(0, C, 3):
                cent[r, c] = x[g.integers(0, na + nb)]
            if C >= 2:
                cent[r, 1] = cent[r, 0]
        return a, b, cent
    return cached(("int", idx), make)


def blob_case(idx):
    def make():
        from dcvgan_amd import evaluation as E
        na, nb, D, C, Rn = SHAPES[idx]
        a, b = R.blobs(60 + idx, na, nb, D, C)
        return a, b, E.prd_host(a, b, C, Rn, T, seed=11 + idx)
    return cached(("blob", idx), make)


def gauss_case(idx):
    def make():
        from dcvgan_amd import evaluation as E
        na, nb, D, C, Rn = GAUSS[idx]
        g = np.random.default_rng(100 + idx)
        a = g.standard_normal((na, D)).astype(F32)
        b = (0.8 * g.standard_normal((nb, D)) + 0.3).astype(F32)
        return a, b, E.prd_host(a, b, C, Rn, T, seed=21 + idx)
    return cached(("gauss", idx), make)


def margin_report(x, norms, cent):
    """Over every row and run: (worst non-tie margin (score_c - best) / (|x|^2 + max cn), exact ties, ties between centroids that are not both integer)."""
    from dcvgan_amd import evaluation as E
    worst, ties, bad = np.inf, 0, 0
    rows = np.arange(x.shape[0])
    for r in range(cent.shape[0]):
        if cent.shape[1] < 2:
            continue
        cn = E._norms_host(cent[r])
        score = cn[None, :] - 2.0 * (x @ cent[r].T)
        best = score.argmin(axis=1)
        gap = score - score[rows, best][:, None]
        other = np.ones_like(gap, dtype=bool)
        other[rows, best] = False
        tie = other & (gap == 0.0)
        whole = (cent[r] == np.rint(cent[r])).all(axis=1)
        ties += int(tie.sum())
        bad += int((tie & ~(whole[None, :] & whole[best][:, None])).sum())
        rel = gap / (norms[:, None] + np.maximum(cn[None, :], cn[best][:, None]))
        sel = other & ~tie
        if sel.any():
            worst = min(worst, float(rel[sel].min()))
    return worst, ties, bad


def layouts(a, b, dev):
    """The two sides as stored: contiguous (16-byte reads where D allows), a row stride of D + 3 with NaN padding, and a base one float into an allocation."""
    return (("contiguous", to_dev(a, dev), to_dev(b, dev)), ("stride D + 3", strided(a, 3, dev), strided(b, 3, dev)), ("base + one float", shifted(a, dev), to_dev(b, dev)))


# ---- seeding ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("na,nb,D,C,Rn,pad", [(70, 65, 16, 20, 10, 0), (5, 4, 3, 9, 2, 0), (33, 40, 7, 5, 3, 2)])
def test_seed_gathers_the_mirrors_rows(dev, na, nb, D, C, Rn, pad):
    from dcvgan_amd import evaluation as E
    g = np.random.default_rng(na)
    a, b = g.standard_normal((na, D)).astype(F32), g.standard_normal((nb, D)).astype(F32)
    a_d, b_d = (strided(a, pad, dev), strided(b, pad + 1, dev)) if pad else (to_dev(a, dev), to_dev(b, dev))
    l0 = E.launches()
    cent = E.prd_seed(a_d, b_d, C, Rn, seed=9)
    assert E.launches() - l0 == 1 and cent.dtype.is_floating_point and tuple(cent.shape) == (Rn, C, D)
    rows = E.prd_seed_host(9, Rn, C, na + nb)
    assert (rows >= na).any() and (rows < na).any()                              # both sides are drawn from
    assert np.array_equal(cent.cpu().numpy(), np.concatenate([a, b]).astype(F64)[rows])


# ---- assignment ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", range(len(SHAPES)))
def test_assign_on_integers_equals_the_mirror_on_both_read_forms(dev, idx):
    from dcvgan_amd import evaluation as E
    a, b, cent = integer_case(idx)
    x, norms = union(a, b)
    want = E._prd_assign_host(x, norms, cent)
    _, ties, _ = margin_report(x, norms, cent)
    print(f"\n[prd assign int] {SHAPES[idx]}: {ties} exact ties")
    if cent.shape[1] >= 2:
        assert ties >= cent.shape[0]                                            # the inputs do hold "the lowest index"
        assert (want == 0).any() and not (want == 1).any()                      # the duplicate never wins
    cent_d = to_dev(cent, dev)
    for what, a_d, b_d in layouts(a, b, dev):
        l0 = E.launches()
        got = E.prd_assign(a_d, b_d, cent_d)
        assert E.launches() - l0 == 4                                           # two norms, cn, the sweep
        assert got.dtype == __import__("torch").int32 and np.array_equal(got.cpu().numpy(), want), (what, np.argwhere(got.cpu().numpy() != want)[:8])
    na_, nb_ = E.row_norms(to_dev(a, dev)), E.row_norms(to_dev(b, dev))
    l0 = E.launches()
    assert np.array_equal(E.prd_assign(to_dev(a, dev), to_dev(b, dev), cent_d, na_, nb_).cpu().numpy(), want) and E.launches() - l0 == 2


# ---- update -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", range(len(SHAPES)))
def test_update_on_integers_equals_the_mirror_for_every_row_split(dev, idx):
    from dcvgan_amd import evaluation as E, native
    na, nb, D, C, Rn = SHAPES[idx]
    a, b, _ = integer_case(idx)
    x, norms = union(a, b)
    g = np.random.default_rng(80 + idx)
    assign = g.integers(0, C + 1, size=(Rn, na + nb)).astype(np.int32)          # C: unassigned
    if C >= 2:
        assign[assign == C - 1] = 0                                              # an empty cluster in every run
        assign[0][assign[0] == 0] = 1 if C > 2 else C                            # and another in run 0
    cent = g.standard_normal((Rn, C, D))                                         # fractions: an untouched centroid is recognisable by its bits
    want_c, want_h = E._prd_update_host(x, norms, na, assign, cent)
    assert want_h[:, :, C].any() and (C < 2 or ((want_h[:, 0] + want_h[:, 1])[:, :C] == 0).any())
    S0 = native.lib().dcv_eval_prd_update_workspace_bytes(na + nb, D, C, Rn, 0) // (Rn * C * D * 8)
    print(f"\n[prd update int] {SHAPES[idx]}: the library's own choice S = {S0}")
    assert S0 >= 1 and (idx != 2 or S0 >= 2)
    assign_d = to_dev(assign, dev)
    for what, a_d, b_d in layouts(a, b, dev):
        for S in (1, 2, 3, 64, 0):
            cent_d = to_dev(cent, dev)
            l0 = E.launches()
            hist = E.prd_update(a_d, b_d, assign_d, cent_d, S)
            assert E.launches() - l0 == 5                                        # two norms, counts, slab sums, fold
            assert np.array_equal(hist.cpu().numpy(), want_h) and hist.cpu().numpy().dtype == np.int32, (what, S)
            got = cent_d.cpu().numpy()
            assert np.array_equal(got, want_c), (what, S, np.argwhere(got != want_c)[:8])
            empty = (want_h[:, 0] + want_h[:, 1])[:, :C] == 0
            assert np.array_equal(got[empty], cent[empty])                       # an empty cluster's centroid is untouched
    na_, nb_ = E.row_norms(to_dev(a, dev)), E.row_norms(to_dev(b, dev))
    assert np.array_equal(E.prd_count(assign_d, na_, nb_, C).cpu().numpy(), want_h)


# ---- the whole k-means --------------------------------------------------------------------------------------------------------------------------------------
def device_trajectory(a_d, b_d, C, Rn, iters, seed):
    """prd_kmeans step by step, everything read back after every step (the test's own reads; prd_kmeans itself reads nothing)."""
    from dcvgan_amd import evaluation as E
    na_, nb_ = E.row_norms(a_d), E.row_norms(b_d)
    cent = E.prd_seed(a_d, b_d, C, Rn, seed)
    assigns, cents, hists = [], [], []
    for t in range(iters + 1):
        cents.append(cent.cpu().numpy().copy())
        assign = E.prd_assign(a_d, b_d, cent, na_, nb_)
        assigns.append(assign.cpu().numpy())
        hist = E.prd_update(a_d, b_d, assign, cent, 0, na_, nb_) if t < iters else E.prd_count(assign, na_, nb_, C)
        hists.append(hist.cpu().numpy())
    return assigns, cents, hists


@pytest.mark.parametrize("idx", range(len(SHAPES)))
def test_kmeans_on_integer_blobs_follows_the_mirror_bit_for_bit(dev, idx):
    from dcvgan_amd import evaluation as E
    na, nb, D, C, Rn = SHAPES[idx]
    a, b, h = blob_case(idx)
    x, norms = union(a, b)
    worst, ties = np.inf, []
    for t in range(T + 1):                                                       # the condition on the inputs: every row, run and iteration
        w, n_ties, bad = margin_report(x, norms, h["cent"][t])
        assert bad == 0, f"iteration {t}: {bad} exact ties between centroids that are not integer"
        worst, ties = min(worst, w), ties + [n_ties]
    fixed = next(t for t in range(1, T + 1) if np.array_equal(h["assign"][t], h["assign"][t - 1]))
    print(f"\n[prd kmeans int] {SHAPES[idx]}: worst non-tie margin {worst:.2e}, exact ties per iteration {ties}, fixed point at iteration {fixed}; mirror "
          f"F8 {h['prd_f8']:.6f}, F1/8 {h['prd_f1_8']:.6f}")
    assert worst >= 1e-9 and fixed < T
    a_d, b_d = to_dev(a, dev), to_dev(b, dev)
    assigns, cents, hists = device_trajectory(a_d, b_d, C, Rn, T, 11 + idx)
    for t in range(T + 1):
        assert np.array_equal(cents[t], h["cent"][t]), (t, "cent")
        assert np.array_equal(assigns[t], h["assign"][t]), (t, "assign", np.argwhere(assigns[t] != h["assign"][t])[:8])
        assert np.array_equal(hists[t], h["hist"][t]), (t, "hist")
    l0 = E.launches()
    hist, cent = E.prd_kmeans(a_d, b_d, C, Rn, T, seed=11 + idx)
    assert E.launches() - l0 == E.prd_launches(T) == 2 + 1 + 5 * T + 3
    assert np.array_equal(hist.cpu().numpy(), h["hist"][-1]) and np.array_equal(cent.cpu().numpy(), h["cent"][-1])
    m = E.prd_metrics(strided(a, 3, dev), shifted(b, dev), C, Rn, T, seed=11 + idx, row_splits=2)
    assert sorted(m) == ["prd_f1_8", "prd_f8"] and all(isinstance(v, float) for v in m.values())
    assert m == {"prd_f8": h["prd_f8"], "prd_f1_8": h["prd_f1_8"]}, (m, h["prd_f8"], h["prd_f1_8"])


@pytest.mark.parametrize("idx", range(len(GAUSS)))
def test_gaussian_features_step_by_step_on_the_mirrors_centroids(dev, idx):
    """Reals g, fakes 0.8 g + 0.3.  From the mirror's centroids of every iteration: the device's assignments equal the mirror's (the margin condition asserted
    first), and the updated centroids lie within 2 (m - 1) eps sum|x_u[d]| / m + eps |c| of the mirror's (m: the cluster's rows; eps = 2^-52: two sums of m terms in
    different orders, each at most (m - 1) eps sum|x|, and the two divisions' rounding).  Over the device's own trajectory the histograms and the two scores are equal.
    Measured on MI355X: see DESIGN §18."""
    from dcvgan_amd import evaluation as E
    na, nb, D, C, Rn = GAUSS[idx]
    a, b, h = gauss_case(idx)
    x, norms = union(a, b)
    worst = min(margin_report(x, norms, h["cent"][t])[0] for t in range(T + 1))
    assert all(margin_report(x, norms, h["cent"][t])[1] == 0 for t in (0, T))
    print(f"\n[prd gauss] {GAUSS[idx]}: worst margin {worst:.2e}; mirror F8 {h['prd_f8']:.6f}, F1/8 {h['prd_f1_8']:.6f}")
    assert worst >= 1e-9
    a_d, b_d = to_dev(a, dev), to_dev(b, dev)
    na_, nb_ = E.row_norms(a_d), E.row_norms(b_d)
    worst_ratio, worst_abs = 0.0, 0.0
    for t in range(T):
        cent_d = to_dev(h["cent"][t], dev)
        assign = E.prd_assign(a_d, b_d, cent_d, na_, nb_)
        assert np.array_equal(assign.cpu().numpy(), h["assign"][t]), t
        hist = E.prd_update(a_d, b_d, assign, cent_d, 0, na_, nb_)
        assert np.array_equal(hist.cpu().numpy(), h["hist"][t]), t
        got, want = cent_d.cpu().numpy(), h["cent"][t + 1]
        bar = np.zeros_like(want)
        for r in range(Rn):
            for c in range(C):
                rows = np.flatnonzero(h["assign"][t][r] == c)
                m = rows.size
                bar[r, c] = (2.0 * (m - 1) * EPS * np.abs(x[rows]).sum(axis=0) / m if m else 0.0) + EPS * np.abs(want[r, c])
        diff = np.abs(got - want)
        worst_abs = max(worst_abs, float(diff.max()))
        worst_ratio = max(worst_ratio, float((diff / np.where(bar > 0, bar, 1.0)).max()))
        assert (diff <= bar).all(), (t, float((diff / np.where(bar > 0, bar, 1.0)).max()))
    print(f"[prd gauss] worst |device - mirror| of a centroid coordinate {worst_abs:.2e}, {worst_ratio:.3f} of its bar")
    assigns, cents, hists = device_trajectory(a_d, b_d, C, Rn, T, 21 + idx)
    drift = max(float(np.abs(cents[t] - h["cent"][t]).max()) for t in range(T + 1))
    print(f"[prd gauss] the device's own trajectory: worst centroid difference {drift:.2e}")
    for t in range(T + 1):
        assert np.array_equal(hists[t], h["hist"][t]) and np.array_equal(assigns[t], h["assign"][t]), t
    assert E.prd_metrics(a_d, b_d, C, Rn, T, seed=21 + idx) == {"prd_f8": h["prd_f8"], "prd_f1_8": h["prd_f1_8"]}


# ---- properties that need no mirror -------------------------------------------------------------------------------------------------------------------------
def test_equal_sides_far_apart_sides_and_the_same_call_twice(dev):
    from dcvgan_amd import evaluation as E
    a, b, _ = gauss_case(0)
    a_d, b_d = to_dev(a, dev), to_dev(b, dev)
    hist, _ = E.prd_kmeans(a_d, a_d, 20, 10, T, seed=3)
    hn = hist.cpu().numpy()
    assert np.array_equal(hn[:, 0], hn[:, 1]) and not hn[:, :, 20].any()
    m = E.prd_metrics(a_d, a_d, 20, 10, T, seed=3)
    assert abs(m["prd_f8"] - 1.0) <= 1e-9 and abs(m["prd_f1_8"] - 1.0) <= 1e-9
    g = np.random.default_rng(5)
    far_a = (100 + g.integers(-2, 3, size=(70, 16))).astype(F32)
    far_b = (-100 + g.integers(-2, 3, size=(65, 16))).astype(F32)
    hist, _ = E.prd_kmeans(to_dev(far_a, dev), to_dev(far_b, dev), 4, 3, T, seed=1)
    hn = hist.cpu().numpy()
    assert not (hn[:, 0, :4] * hn[:, 1, :4]).any()                               # no cluster holds both sides
    assert E.prd_metrics(to_dev(far_a, dev), to_dev(far_b, dev), 4, 3, T, seed=1) == {"prd_f8": 0.0, "prd_f1_8": 0.0}
    h1, c1 = E.prd_kmeans(a_d, b_d, 20, 10, T, seed=4)
    h1, c1 = h1.cpu().numpy().copy(), c1.cpu().numpy().copy()
    h2, c2 = E.prd_kmeans(a_d, b_d, 20, 10, T, seed=4)
    assert np.array_equal(h1, h2.cpu().numpy()) and np.array_equal(c1.view(np.int64), c2.cpu().numpy().view(np.int64))
    h3, _ = E.prd_kmeans(a_d, b_d, 20, 10, T, seed=5)
    assert not np.array_equal(h1, h3.cpu().numpy())


# ---- non-finite ---------------------------------------------------------------------------------------------------------------------------------------------
def test_a_non_finite_row_is_unassigned_and_the_scores_are_nan(dev):
    from dcvgan_amd import evaluation as E
    na, nb, D, C, Rn = SHAPES[0]
    a, b, cent = integer_case(0)
    a, b = a.copy(), b.copy()
    a[5, 3] = np.nan
    b[64, 0] = np.inf
    x, norms = union(a, b)
    a_d, b_d = to_dev(a, dev), to_dev(b, dev)
    got = E.prd_assign(a_d, b_d, to_dev(cent, dev)).cpu().numpy()
    bad = np.array([5, na + 64])
    assert (got[:, bad] == C).all()
    keep = np.ones(na + nb, dtype=bool)
    keep[bad] = False
    assert np.array_equal(got[:, keep], E._prd_assign_host(x[keep], norms[keep], cent)) and (got[:, keep] < C).all()
    assert np.array_equal(got, E._prd_assign_host(x, norms, cent))
    # an update leaves the rows out although the explicit assignment names a cluster for them: no 0 * NaN reaches any sum
    assign = np.zeros((Rn, na + nb), dtype=np.int32)
    cent_d = to_dev(cent, dev)
    hist = E.prd_update(a_d, b_d, to_dev(assign, dev), cent_d).cpu().numpy()
    want_c, want_h = E._prd_update_host(x, norms, na, assign, cent)
    assert np.array_equal(hist, want_h) and np.array_equal(hist[:, :, C], np.ones((Rn, 2), dtype=np.int32))
    assert np.array_equal(cent_d.cpu().numpy(), want_c) and np.isfinite(want_c).all()
    h = E.prd_host(a, b, C, Rn, T, seed=2)
    hist, cent_k = E.prd_kmeans(a_d, b_d, C, Rn, T, seed=2)
    assert np.array_equal(hist.cpu().numpy()[:, :, C], np.ones((Rn, 2), dtype=np.int32)) and np.array_equal(hist.cpu().numpy(), h["hist"][-1])
    m = E.prd_metrics(a_d, b_d, C, Rn, T, seed=2)
    assert sorted(m) == ["prd_f1_8", "prd_f8"] and all(np.isnan(v) for v in m.values()) and np.isnan(h["prd_f8"])


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------------------------
def test_evaluator_reports_the_two_scores(dev):
    """Generators of the smallest configuration the suite builds; 12 real clips, 70 samples in batches of 10.  The extractor returns free views of the clip."""
    import torch
    from dcvgan_amd import evaluation as E, native, trainer
    cfg = rig.small_cfg()
    models, _ = rig.seeded_models(cfg, dev, cfg.seed, 123)

    def extractor(xc):
        flat = xc.permute(0, 2, 1, 3, 4).reshape(xc.shape[0], -1)
        return flat[:, :24], None

    g = torch.Generator().manual_seed(3)
    reals = [(torch.rand(4, 3, 16, 64, 64, generator=g) * 2 - 1).to(dev) for _ in range(3)]
    kw = dict(prd_clusters=5, prd_runs=3, prd_iters=4, seed=5, max_features=80)
    for metrics in (("prcurve",), ("kid", "pr", "prcurve")):
        ev = trainer.build_evaluator(cfg, models, extractor, metrics=metrics, kid_subsets=3, kid_subset_size=4, **kw)
        assert (ev.prd_clusters, ev.prd_runs, ev.prd_iters) == (5, 3, 4) and ev.real is None
        l0, n0 = E.launches(), native.launch_count()
        with pytest.raises(native.NativeError, match='"prcurve"' if metrics == ("prcurve",) else '"kid"'):
            ev.evaluate(num_samples=70, batchsize=10)                            # no real features yet: refused before anything launches
        assert E.launches() == l0 and native.launch_count() == n0
        for xr in reals:
            ev.observe_real(xr)
        assert ev.n_real_feats == 12
        l0 = E.launches()
        out = ev.evaluate(num_samples=70, batchsize=10)
        others = 0 if metrics == ("prcurve",) else 3 + E.manifold_launches(3, 5, ("pr",))
        assert E.launches() - l0 == 7 + others + E.prd_launches(4)               # seven stores, then the metrics
        keys = ["prd_f1_8", "prd_f8"] + ([] if metrics == ("prcurve",) else ["kid", "kid_std", "precision", "recall"])
        assert sorted(out) == sorted(keys) and all(isinstance(v, float) for v in out.values()) and ev.n_fake_feats == 70
        real, fake = ev.real_feats[:12], ev.fake_feats[:70]
        want = E.prd_metrics(real, fake, 5, 3, 4, seed=5)
        print(f"\n[evaluate {metrics}] {out}")
        assert {key: out[key] for key in want} == want and 0.0 <= out["prd_f8"] <= 1.0 and 0.0 <= out["prd_f1_8"] <= 1.0
        hm = E.prd_host(real.cpu().numpy(), fake.cpu().numpy(), 5, 3, 4, seed=5)
        print(f"[evaluate] mirror: F8 {hm['prd_f8']}, F1/8 {hm['prd_f1_8']}")
        # a second evaluation fills the same buffers
        ptrs = (ev.real_feats.data_ptr(), ev.fake_feats.data_ptr())
        first = fake.cpu().numpy().copy()
        out2 = ev.evaluate(num_samples=70, batchsize=10)
        assert (ev.real_feats.data_ptr(), ev.fake_feats.data_ptr()) == ptrs and ev.n_fake_feats == 70 and ev.n_real_feats == 12
        assert not np.array_equal(ev.fake_feats[:70].cpu().numpy(), first)
        assert {key: out2[key] for key in want} == E.prd_metrics(ev.real_feats[:12], ev.fake_feats[:70], 5, 3, 4, seed=5)
