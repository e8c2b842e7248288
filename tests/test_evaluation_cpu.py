"""CPU: the evaluation statistics' binding, their refusals, and the host half of the metrics.

`gram_ref`, `inception_ref` and `kid_ref` are the numpy restatements tests/test_evaluation_gpu.py holds the kernels to; here the host arithmetic is checked on its
own: the Fréchet distance against the scipy.linalg.sqrtm formulation, the draw's mirror, the Inception score's finalisation, the save / load round trip."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dcv_eval_moments_update", "dcv_eval_inception_workspace_bytes", "dcv_eval_inception_update", "dcv_eval_kid_draw", "dcv_eval_kid_workspace_bytes",
       "dcv_eval_kid_sums")
F32, F64 = np.float32, np.float64
EPS = 2.0 ** -53      # the unit roundoff of fp64: one rounded operation is off by at most EPS relative


# ---- the restatements ---------------------------------------------------------------------------------------------------------------------------------------
def gram_ref(x):
    """(sum, gram) of fp32 rows in numpy fp64: products of fp32 values are exact there, the sums carry numpy's own order."""
    x = np.asarray(x, dtype=F32).astype(F64)
    return x.sum(axis=0), x.T @ x


def inception_ref(logits):
    """state (K + 1,) of dcv_eval_inception_update from zero, operation by operation: m = max; e = exp(z - m); S = sum e; p = e / S; log p = (z - m) - log S;
    state[:K] = sum_i p_i; state[K] = sum_i sum_k p log p with p == 0 adding nothing.  (numpy's summation order, not the kernel's: the bar of the GPU test covers it.)"""
    z = np.asarray(logits, dtype=F32).astype(F64)
    with np.errstate(all="ignore"):
        d = z - z.max(axis=1, keepdims=True)
        e = np.exp(d)
        S = e.sum(axis=1, keepdims=True)
        p = e / S
        lp = d - np.log(S)
        term = np.where(p == 0.0, 0.0, p * lp)
    return np.concatenate([p.sum(axis=0), [term.sum()]])


def kid_ref(fa, fb, table, exact=False):
    """out (subsets, 3) of dcv_eval_kid_sums: t = dot / D + 1, (t * t) * t, the diagonal of the two symmetric blocks left out.  exact: integer features with D a
    power of two — everything in int64 (scaled by D^3), then one exact division."""
    fa, fb, table = np.asarray(fa, dtype=F32), np.asarray(fb, dtype=F32), np.asarray(table)
    D = fa.shape[1]
    out = []
    for s in range(table.shape[0]):
        a, b = fa[table[s, 0]], fb[table[s, 1]]
        row = []
        for u, v, sym in ((a, a, True), (b, b, True), (a, b, False)):
            if exact:
                dot = u.astype(np.int64) @ v.astype(np.int64).T
                k = (dot + D) ** 3                                   # D^3 (dot / D + 1)^3, an integer
            else:
                dot = u.astype(F64) @ v.astype(F64).T
                t = dot / F64(D) + 1.0
                k = (t * t) * t
            if sym:
                k = k - np.diag(np.diag(k))
            row.append(k.sum())
        out.append(row)
    out = np.array(out)
    return out.astype(F64) / F64(D) ** 3 if exact else out.astype(F64)


def abs_kid_ref(fa, fb, table):
    """sum |k_ij| per (subset, block): the scale of the real-valued bar."""
    fa, fb, table = np.asarray(fa, dtype=F32).astype(F64), np.asarray(fb, dtype=F32).astype(F64), np.asarray(table)
    D = fa.shape[1]
    k = lambda u, v: np.abs((u @ v.T / D + 1.0) ** 3)
    return np.array([[k(fa[t[0]], fa[t[0]]).sum(), k(fb[t[1]], fb[t[1]]).sum(), k(fa[t[0]], fb[t[1]]).sum()] for t in table])


def fid_sqrtm(mu_a, sa, mu_b, sb):
    """The usual formulation: |mu_a - mu_b|^2 + tr(S_a + S_b - 2 sqrtm(S_a S_b))."""
    from scipy import linalg
    covmean = linalg.sqrtm(sa @ sb)
    d = mu_a - mu_b
    return float(d @ d + np.trace(sa) + np.trace(sb) - 2.0 * np.trace(covmean.real))


def moments_of(x):
    """A host-only FeatureMoments holding the numpy statistics of the rows x."""
    from dcvgan_amd import evaluation as E
    x = np.asarray(x, dtype=F64)
    fm = E.FeatureMoments(x.shape[1], device="cpu")
    return fm.load_state_dict(dict(dim=x.shape[1], n=x.shape[0], sum=x.sum(axis=0), gram=x.T @ x))


# ---- the binding --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from dcvgan_amd import native
    if not os.path.exists(native.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return native.lib()


def test_new_names_are_bound_declared_and_exported(lib):
    from dcvgan_amd import evaluation, native, trainer
    header = open(os.path.join(ROOT, "include", "dcvgan_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    raw = ctypes.CDLL(native.LIB_PATH)
    for n in NEW:
        assert n in native.EXPORTS, n
        assert re.search(r"\b%s\s*\(" % n, code), f"{n} is not declared in dcvgan_hip.h"
        assert hasattr(raw, n), f"{n} is not exported by the library"
    assert lib.dcv_version() == native.ABI_VERSION == 4
    assert re.search(r"#define\s+DCV_EVAL_KID_SALT\s+0x%Xull" % evaluation.KID_SALT, header)
    assert re.search(r"for f in [^;]*\bevalstats\b", open(os.path.join(ROOT, "dcvgan_amd", "csrc", "build.sh")).read()), "csrc/evalstats.hip is not in build.sh's list"
    assert callable(trainer.build_evaluator) and evaluation.launches() >= 0
    p = inspect.signature(evaluation.kernel_distance).parameters
    assert (p["num_subsets"].default, p["subset_size"].default, p["seed"].default, p["table"].default) == (100, 1000, 0, None)
    assert inspect.signature(evaluation.Evaluator.__init__).parameters["metrics"].default == ("is", "fid", "kid")


def test_refusals_need_no_gpu(lib, tmp_path):
    """The argument checks run on the host before any launch."""
    import torch
    from dcvgan_amd import evaluation as E, native
    buf = ctypes.create_string_buffer(256)      # never dereferenced
    a = (ctypes.addressof(buf) + 15) // 16 * 16
    n0 = lib.dcv_launch_count()
    EINVAL = native.DCV_EINVAL

    mom = lambda x=a, n=4, D=8, stride=8, s=a, g=a: lib.dcv_eval_moments_update(x, n, D, stride, s, g, None)
    assert mom(x=None) == EINVAL and mom(s=None) == EINVAL and mom(g=None) == EINVAL and mom(s=a + 4) == EINVAL
    assert mom(D=0) == EINVAL and mom(D=4097, stride=4097) == EINVAL and b"4096" in lib.dcv_last_error()
    assert mom(n=0) == EINVAL and mom(n=2 ** 31) == EINVAL and b"2^31" in lib.dcv_last_error()
    assert mom(stride=7) == EINVAL and b"row_stride" in lib.dcv_last_error()

    assert lib.dcv_eval_inception_workspace_bytes(70, 400) == 70 * 401 * 8 and lib.dcv_eval_inception_workspace_bytes(10 ** 6, 4096) == 256 * 4097 * 8
    assert lib.dcv_eval_inception_workspace_bytes(0, 4) == 0 and lib.dcv_eval_inception_workspace_bytes(4, 4097) == 0
    inc = lambda z=a, n=4, K=8, stride=8, st=a, ws=a, nb=1 << 20: lib.dcv_eval_inception_update(z, n, K, stride, st, ws, nb, None)
    assert inc(z=None) == EINVAL and inc(st=None) == EINVAL and inc(ws=None) == EINVAL
    assert inc(K=0) == EINVAL and inc(K=4097, stride=4097) == EINVAL and inc(n=0) == EINVAL and inc(n=2 ** 31) == EINVAL and inc(stride=7) == EINVAL
    assert inc(nb=4 * 9 * 8 - 1) == native.DCV_EWORKSPACE and b"workspace" in lib.dcv_last_error()

    draw = lambda t=a, subsets=3, m=5, na=9, nb=7: lib.dcv_eval_kid_draw(t, subsets, m, na, nb, 0, None)
    assert draw(t=None) == EINVAL and draw(subsets=0) == EINVAL and draw(subsets=4097) == EINVAL and draw(m=1) == EINVAL and draw(m=65537, na=10 ** 6, nb=10 ** 6) == EINVAL
    assert draw(na=4) == EINVAL and draw(nb=4) == EINVAL and draw(na=2 ** 31) == EINVAL

    assert lib.dcv_eval_kid_workspace_bytes(3, 33) == 3 * (1 + 1 + 1) * 8 and lib.dcv_eval_kid_workspace_bytes(100, 1000) == 100 * (136 + 136 + 256) * 8
    assert lib.dcv_eval_kid_workspace_bytes(0, 5) == 0 and lib.dcv_eval_kid_workspace_bytes(1, 1) == 0 and lib.dcv_eval_kid_workspace_bytes(1, 65537) == 0
    kid = lambda fa=a, sa=16, na=9, fb=a, sb=16, nb=7, D=16, t=a, subsets=3, m=5, ws=a, wb=1 << 20, out=a: \
        lib.dcv_eval_kid_sums(fa, sa, na, fb, sb, nb, D, t, subsets, m, ws, wb, out, None)
    assert kid(fa=None) == EINVAL and kid(fb=None) == EINVAL and kid(t=None) == EINVAL and kid(ws=None) == EINVAL and kid(out=None) == EINVAL
    assert kid(m=1) == EINVAL and kid(m=65537) == EINVAL and kid(subsets=0) == EINVAL and kid(subsets=4097) == EINVAL
    assert kid(D=0) == EINVAL and kid(D=4097, sa=4097, sb=4097) == EINVAL and kid(sa=15) == EINVAL and kid(sb=15) == EINVAL and b"stride" in lib.dcv_last_error()
    assert kid(na=0) == EINVAL and kid(nb=2 ** 31) == EINVAL
    assert kid(wb=3 * 3 * 8 - 1) == native.DCV_EWORKSPACE
    assert lib.dcv_launch_count() == n0

    # Python: anything that is not a (n, D) fp32 device tensor is refused; so is a metric whose inputs are missing, by name
    l0 = E.launches()
    fm, st = E.FeatureMoments(8, device="cpu"), E.InceptionStats(5, device="cpu")
    for bad in (torch.zeros(4, 8), torch.zeros(4, 8, dtype=torch.float64), np.zeros((4, 8), dtype=F32)):
        with pytest.raises(native.NativeError):
            fm.update(bad)
        with pytest.raises(native.NativeError):
            st.update(bad)
    with pytest.raises(native.NativeError):
        E.kernel_distance(torch.zeros(4, 8), torch.zeros(4, 8))
    for bad in (0, 4097):
        with pytest.raises(ValueError):
            E.FeatureMoments(bad, device="cpu")
        with pytest.raises(ValueError):
            E.InceptionStats(bad, device="cpu")
    with pytest.raises(ValueError):
        fm.cov()                                  # n < 2
    with pytest.raises(ValueError):
        E.Evaluator(lambda x: (x, None), metrics=("is", "prd"))
    ev = E.Evaluator(lambda x: (x, None), metrics=("fid",))
    with pytest.raises(native.NativeError, match='"fid"'):
        ev.evaluate(object(), object(), 5, 2)     # no real statistics: refused before the generators are touched
    ev = E.Evaluator(lambda x: (x, None), metrics=("kid",), real_moments=moments_of(np.eye(8)))
    with pytest.raises(native.NativeError, match='"kid"'):
        ev.evaluate(object(), object(), 5, 2)     # real moments alone do not make a kernel distance
    with pytest.raises(native.NativeError):
        ev.observe_real(torch.zeros(2, 3, 4, 8, 8))      # a CPU clip
    with pytest.raises(ValueError):
        E.Evaluator(lambda x: (x, None)).evaluate(None, None, 5, 2)
    assert E.launches() == l0 and lib.dcv_launch_count() == n0


# ---- the Fréchet distance ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,D", [(200, 48), (1000, 256)])
def test_frechet_distance_against_sqrtm(n, D):
    """Full-rank Gaussian features: the eigenvalue route and scipy's sqrtm agree to 1e-10 relative (they agreed to ~1e-14 when tried; the margin is for LAPACK
    builds)."""
    from dcvgan_amd import evaluation as E
    g = np.random.default_rng(100 + D)
    mix = g.standard_normal((D, D)) / np.sqrt(D)
    xa = g.standard_normal((n, D)) @ mix + 0.3
    xb = (g.standard_normal((n + 17, D)) * 1.2) @ mix.T - 0.1
    a, b = moments_of(xa), moments_of(xb)
    got = E.frechet_distance(a, b)
    want = fid_sqrtm(xa.mean(0), np.cov(xa, rowvar=False), xb.mean(0), np.cov(xb, rowvar=False))
    print(f"\n[fid] n {n} D {D}: eigenvalue route {got!r}, sqrtm {want!r}, relative difference {abs(got - want) / abs(want):.1e}")
    assert abs(got - want) <= 1e-10 * abs(want)
    assert abs(E.frechet_distance(a, a)) <= 1e-9 * np.trace(a.cov())
    assert abs(got - E.frechet_distance(b, a)) <= 1e-10 * abs(want)      # symmetric in its arguments


def test_frechet_distance_with_fewer_rows_than_features():
    """n < D: the covariances are singular and sqrtm itself is only good to ~1e-8 there, so no agreement with it is asserted: finite, non-negative, and zero against
    itself to 1e-9 of the trace."""
    from dcvgan_amd import evaluation as E
    g = np.random.default_rng(7)
    xa, xb = g.standard_normal((30, 48)) + 0.5, g.standard_normal((30, 48)) * 0.7
    a, b = moments_of(xa), moments_of(xb)
    f = E.frechet_distance(a, b)
    print(f"\n[fid] n 30 D 48: {f!r}; against itself {E.frechet_distance(a, a)!r}, {E.frechet_distance(b, b)!r} (traces {np.trace(a.cov()):.3g}, {np.trace(b.cov()):.3g})")
    assert np.isfinite(f) and f >= 0.0
    assert abs(E.frechet_distance(a, a)) <= 1e-9 * np.trace(a.cov()) and abs(E.frechet_distance(b, b)) <= 1e-9 * np.trace(b.cov())
    with pytest.raises(ValueError):
        E.frechet_distance(a, moments_of(g.standard_normal((30, 16))))


def test_save_load_round_trip(tmp_path):
    """mean() to 1e-12 relative, element by element.  cov() to 1e-12 of max |cov|, not of each element: the features have mean 3, so an off-diagonal entry is a
    small difference of sums near 9 n and its own size says nothing about the rounding it carries; the largest entry is the scale of every entry's error."""
    from dcvgan_amd import evaluation as E
    g = np.random.default_rng(3)
    x = g.standard_normal((77, 20)) * g.uniform(0.5, 2.0, size=20) + 3.0
    a = moments_of(x)
    assert np.allclose(a.mean(), x.mean(0), rtol=1e-13, atol=0) and np.allclose(a.cov(), np.cov(x, rowvar=False), rtol=0, atol=1e-12)
    path = str(tmp_path / "real_stats.npz")
    a.save(path)
    with np.load(path) as z:
        assert sorted(z.files) == ["mu", "n", "sigma"] and int(z["n"]) == 77 and z["mu"].shape == (20,) and z["sigma"].shape == (20, 20)
    b = E.FeatureMoments.load(path, device="cpu")
    scale = np.abs(a.cov()).max()
    assert b.n == 77 and b.dim == 20
    assert np.all(np.abs(b.mean() - a.mean()) <= 1e-12 * np.abs(a.mean()))
    assert np.all(np.abs(b.cov() - a.cov()) <= 1e-12 * scale)
    sd = a.state_dict()
    c = E.FeatureMoments(20, device="cpu").load_state_dict(sd)
    assert c.n == 77 and np.array_equal(c.cov(), a.cov()) and np.array_equal(c.mean(), a.mean())
    with pytest.raises(ValueError):
        E.FeatureMoments(21, device="cpu").load_state_dict(sd)


# ---- the draw's mirror -----------------------------------------------------------------------------------------------------------------------------------
def test_draw_mirror_subsets_are_distinct_and_in_range():
    from dcvgan_amd import evaluation as E
    for seed, subsets, m, na, nb in ((0, 4, 5, 5, 9), (1, 3, 33, 100, 34), (12345, 2, 1000, 1000, 4097)):
        t = E.draw_host(seed, subsets, m, na, nb)
        assert t.shape == (subsets, 2, m) and t.dtype == np.int32
        for s in range(subsets):
            for side, n_rows in ((0, na), (1, nb)):
                row = t[s, side]
                assert row.min() >= 0 and row.max() < n_rows and len(set(row.tolist())) == m, (seed, s, side)
        assert sorted(t[0, 0].tolist()) == list(range(m)) or m < na       # m == na: a whole permutation
    a, b = E.draw_host(0, 3, 33, 100, 50), E.draw_host(1, 3, 33, 100, 50)
    assert not np.array_equal(a, b)                                        # two seeds differ
    assert not np.array_equal(a[0], a[1]) and not np.array_equal(a[1], a[2])      # two subsets differ
    assert not np.array_equal(a[0, 0], E.draw_host(0, 3, 33, 100, 100)[0, 1])     # and so do the two sides over the same range
    assert np.array_equal(a, E.draw_host(0, 3, 33, 100, 50))
    assert np.array_equal(a[:2], E.draw_host(0, 2, 33, 100, 50))           # a subset depends on (seed, s, side) alone
    for bad in ((0, 0, 5, 9, 9), (0, 1, 1, 9, 9), (0, 1, 5, 4, 9), (0, 1, 5, 9, 2 ** 31)):
        with pytest.raises(ValueError):
            E.draw_host(*bad)


# ---- the Inception score's finalisation --------------------------------------------------------------------------------------------------------------------
def test_inception_score_finalisation():
    from dcvgan_amd import evaluation as E
    n, K = 12, 8
    flat = inception_ref(np.full((n, K), 2.5, dtype=F32))
    assert np.array_equal(flat[:K], np.full(K, n / 8.0))                   # e = 1, S = 8, p = 1/8: exact
    assert abs(E.inception_score_from_state(flat, n) - 1.0) <= 1e-12       # all-equal logits: p(y|x) = p(y), the score is 1
    for K in (2, 7, 400):
        z = np.full((3 * K, K), -80.0, dtype=F32)
        z[np.arange(3 * K), np.arange(3 * K) % K] = 80.0                   # K balanced, confident classes
        s = E.inception_score_from_state(inception_ref(z), 3 * K)
        assert abs(s - K) <= 1e-12 * K, (K, s)
    st = E.InceptionStats(8, device="cpu").load_state_dict(dict(num_classes=8, n=n, state=flat))
    assert abs(st.score() - 1.0) <= 1e-12 and st.state_dict()["n"] == n
    with pytest.raises(ValueError):
        E.inception_score_from_state(flat, 0)


def test_restatements_agree_with_direct_formulas():
    """kid_ref's exact leg equals its floating leg on integer data, and mmd2_from_sums is the unbiased estimator."""
    from dcvgan_amd import evaluation as E
    g = np.random.default_rng(5)
    fa, fb = g.integers(-4, 5, size=(9, 16)).astype(F32), g.integers(-4, 5, size=(7, 16)).astype(F32)
    table = np.stack([np.stack([g.permutation(9)[:5], g.permutation(7)[:5]]) for _ in range(3)]).astype(np.int32)
    assert np.array_equal(kid_ref(fa, fb, table, exact=True), kid_ref(fa, fb, table))
    out = kid_ref(fa, fb, table)
    a, b = fa[table[0, 0]].astype(F64), fb[table[0, 1]].astype(F64)
    k = lambda u, v: (u @ v.T / 16.0 + 1.0) ** 3
    kaa, kbb, kab = k(a, a), k(b, b), k(a, b)
    m = 5
    want = (kaa.sum() - np.trace(kaa)) / (m * (m - 1)) + (kbb.sum() - np.trace(kbb)) / (m * (m - 1)) - 2 * kab.mean()
    assert abs(E.mmd2_from_sums(out, m)[0] - want) <= 1e-12 * abs(want)
