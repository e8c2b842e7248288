"""CPU: the k-nearest-neighbour manifold metrics' binding, their refusals, and the numpy mirror.

`manifold_host` is the specification tests/test_manifold_gpu.py holds the kernels to; here it is checked on its own against a brute-force triple loop over explicit
differences, sum (x - y)^2, on integer features, where both are exact."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dcv_eval_row_norms", "dcv_eval_knn_workspace_bytes", "dcv_eval_knn_radii", "dcv_eval_manifold_workspace_bytes", "dcv_eval_manifold_counts",
       "dcv_eval_manifold_reduce")
F32, F64 = np.float32, np.float64


# ---- the brute force ----------------------------------------------------------------------------------------------------------------------------------------
def brute(a, b, k):
    """The four metrics and what they are counted from, by loops over explicit differences; every comparison <=, self excluded by index."""
    a, b = np.asarray(a, dtype=F64), np.asarray(b, dtype=F64)

    def d2(x, y):
        s = 0.0
        for u, v in zip(x, y):
            s += (u - v) * (u - v)
        return s

    def radii(x):
        out = []
        for i in range(len(x)):
            ds = sorted(d2(x[i], x[j]) for j in range(len(x)) if j != i)
            out.append(ds[k - 1])
        return np.array(out)

    ra, rb = radii(a), radii(b)
    count_ba = np.array([sum(1 for i in range(len(a)) if d2(b[j], a[i]) <= ra[i]) for j in range(len(b))])
    count_ab = np.array([sum(1 for j in range(len(b)) if d2(a[i], b[j]) <= rb[j]) for i in range(len(a))])
    dmin_ba = np.array([min(d2(b[j], a[i]) for i in range(len(a))) for j in range(len(b))])
    dmin_ab = np.array([min(d2(a[i], b[j]) for j in range(len(b))) for i in range(len(a))])
    return dict(rad2_a=ra, rad2_b=rb, count_ba=count_ba, count_ab=count_ab, dmin2_ba=dmin_ba, dmin2_ab=dmin_ab,
                precision=float((count_ba > 0).sum() / len(b)), recall=float((count_ab > 0).sum() / len(a)),
                density=float(count_ba.sum() / (float(k) * len(b))), coverage=float((dmin_ab <= ra).sum() / len(a)))


def same(got, want):
    for key in want:
        assert np.array_equal(np.asarray(got[key]), np.asarray(want[key])), (key, got[key], want[key])


def integer_case(seed, na, nb, D):
    """Integers in [-3, 3] as fp32: every dot, norm and distance is an exact integer in fp64."""
    g = np.random.default_rng(seed)
    return g.integers(-3, 4, size=(na, D)).astype(F32), g.integers(-3, 4, size=(nb, D)).astype(F32)


def ties(a, b, k):
    """How many (query, support) pairs lie exactly ON a ball's surface, d2 == rad2, over both directions: what separates <= from <."""
    from dcvgan_amd import evaluation as E
    h = E.manifold_host(a, b, k)
    return int((E.d2_host(b, a) == h["rad2_a"][None, :]).sum() + (E.d2_host(a, b) == h["rad2_b"][None, :]).sum())


# ---- the binding --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from dcvgan_amd import native
    if not os.path.exists(native.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return native.lib()


def test_new_names_are_bound_declared_and_exported(lib):
    from dcvgan_amd import evaluation, native
    header = open(os.path.join(ROOT, "include", "dcvgan_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    raw = ctypes.CDLL(native.LIB_PATH)
    for n in NEW:
        assert n in native.EXPORTS, n
        assert re.search(r"\b%s\s*\(" % n, code), f"{n} is not declared in dcvgan_hip.h"
        assert hasattr(raw, n), f"{n} is not exported by the library"
    assert lib.dcv_version() == native.ABI_VERSION == 4
    assert re.search(r"for f in [^;]*\bevalknn\b", open(os.path.join(ROOT, "dcvgan_amd", "csrc", "build.sh")).read()), "csrc/evalknn.hip is not in build.sh's list"
    assert "pr" in evaluation.METRICS and "dc" in evaluation.METRICS and evaluation.METRICS[:3] == ("is", "fid", "kid")
    p = inspect.signature(evaluation.manifold_metrics).parameters
    assert (p["k_pr"].default, p["k_dc"].default, p["metrics"].default) == (3, 5, ("pr", "dc"))
    p = inspect.signature(evaluation.Evaluator.__init__).parameters
    assert (p["pr_k"].default, p["dc_k"].default) == (3, 5) and p["metrics"].default == ("is", "fid", "kid")
    assert list(p)[-2:] == ["pr_k", "dc_k"]                                  # after the existing keyword arguments
    assert inspect.signature(evaluation.knn_radii).parameters["col_splits"].default == 0
    assert inspect.signature(evaluation.manifold_counts).parameters["col_splits"].default == 0
    assert (evaluation.manifold_launches(), evaluation.manifold_launches(metrics=("pr",)), evaluation.manifold_launches(metrics=("dc",)),
            evaluation.manifold_launches(4, 4)) == (17, 12, 10, 12)
    assert "<=" in evaluation.manifold_metrics.__doc__ and "prdc" in evaluation.manifold_metrics.__doc__


def test_refusals_need_no_gpu(lib):
    """The argument checks run on the host before any launch."""
    import torch
    from dcvgan_amd import evaluation as E, native
    buf = ctypes.create_string_buffer(256)      # never dereferenced
    a = (ctypes.addressof(buf) + 15) // 16 * 16
    n0 = lib.dcv_launch_count()
    EINVAL, EWS = native.DCV_EINVAL, native.DCV_EWORKSPACE

    nrm = lambda x=a, n=9, D=8, stride=8, o=a: lib.dcv_eval_row_norms(x, n, D, stride, o, None)
    assert nrm(x=None) == EINVAL and nrm(o=None) == EINVAL and nrm(o=a + 4) == EINVAL
    assert nrm(D=0) == EINVAL and nrm(D=4097, stride=4097) == EINVAL and b"4096" in lib.dcv_last_error()
    assert nrm(n=0) == EINVAL and nrm(n=2 ** 31) == EINVAL and nrm(stride=7) == EINVAL and b"row_stride" in lib.dcv_last_error()

    # S * n * k * 8 bytes; S = col_splits, or for 0 max(1, min(64, column tiles, 512 / row tiles)) with tiles of 64
    wk = lib.dcv_eval_knn_workspace_bytes
    assert wk(130, 5, 2) == 2 * 130 * 5 * 8 and wk(130, 5, 64) == 64 * 130 * 5 * 8
    assert wk(130, 5, 0) == 3 * 130 * 5 * 8                                   # 3 column tiles
    assert wk(10000, 3, 0) == 3 * 10000 * 3 * 8                               # 157 row tiles: 512 / 157 = 3
    assert wk(50000, 16, 0) == 1 * 50000 * 16 * 8                             # 782 row tiles: one share
    assert wk(4, 3, 0) == 4 * 3 * 8
    assert wk(3, 3, 0) == 0 and wk(9, 0, 0) == 0 and wk(99, 17, 0) == 0 and wk(2 ** 31, 3, 0) == 0 and wk(9, 3, 65) == 0 and wk(9, 3, -1) == 0
    knn = lambda x=a, n=9, D=8, stride=8, nm=a, k=3, cs=0, ws=a, wb=1 << 20, r=a: lib.dcv_eval_knn_radii(x, n, D, stride, nm, k, cs, ws, wb, r, None)
    assert knn(x=None) == EINVAL and knn(nm=None) == EINVAL and knn(ws=None) == EINVAL and knn(r=None) == EINVAL
    assert knn(nm=a + 4) == EINVAL and knn(r=a + 4) == EINVAL and b"misaligned" in lib.dcv_last_error()
    assert knn(D=0) == EINVAL and knn(D=4097, stride=4097) == EINVAL
    assert knn(k=0) == EINVAL and knn(k=17, n=99) == EINVAL and b"16" in lib.dcv_last_error()
    assert knn(n=3) == EINVAL and b"k + 1" in lib.dcv_last_error() and knn(n=2 ** 31) == EINVAL
    assert knn(stride=7) == EINVAL and knn(cs=-1) == EINVAL and knn(cs=65) == EINVAL and b"col_splits" in lib.dcv_last_error()
    assert knn(wb=9 * 3 * 8 - 1) == EWS and b"workspace" in lib.dcv_last_error() and knn(cs=4, wb=4 * 9 * 3 * 8 - 1) == EWS

    # S * nq * 12 bytes: a double and an int32 per query and share; S over the SUPPORT's column tiles
    wm = lib.dcv_eval_manifold_workspace_bytes
    assert wm(97, 130, 2) == 2 * 97 * 12 and wm(97, 130, 0) == 3 * 97 * 12 and wm(130, 97, 0) == 2 * 130 * 12 and wm(10000, 10000, 0) == 3 * 10000 * 12
    assert wm(0, 5, 0) == 0 and wm(5, 0, 0) == 0 and wm(2 ** 31, 5, 0) == 0 and wm(5, 2 ** 31, 0) == 0 and wm(5, 5, 65) == 0 and wm(5, 5, -1) == 0
    cnt = lambda q=a, sq=8, nq=9, qn=a, s=a, ss=8, ns=7, sn=a, r=a, D=8, cs=0, ws=a, wb=1 << 20, c=a, m=a: \
        lib.dcv_eval_manifold_counts(q, sq, nq, qn, s, ss, ns, sn, r, D, cs, ws, wb, c, m, None)
    assert cnt(q=None) == EINVAL and cnt(qn=None) == EINVAL and cnt(s=None) == EINVAL and cnt(sn=None) == EINVAL and cnt(ws=None) == EINVAL
    assert cnt(c=None) == EINVAL and cnt(m=None) == EINVAL and cnt(m=a + 4) == EINVAL and cnt(r=a + 4) == EINVAL and cnt(qn=a + 4) == EINVAL
    assert cnt(D=0) == EINVAL and cnt(D=4097, sq=4097, ss=4097) == EINVAL and cnt(sq=7) == EINVAL and cnt(ss=7) == EINVAL and b"stride" in lib.dcv_last_error()
    assert cnt(nq=0) == EINVAL and cnt(ns=0) == EINVAL and cnt(nq=2 ** 31) == EINVAL and cnt(ns=2 ** 31) == EINVAL
    assert cnt(nq=2 ** 27, ns=2 ** 26) == EINVAL and b"2^53" in lib.dcv_last_error()
    assert cnt(cs=65) == EINVAL and cnt(cs=-1) == EINVAL
    assert cnt(wb=9 * 12 - 1) == EWS and cnt(cs=5, wb=5 * 9 * 12 - 1) == EWS

    red = lambda c=a, m=a, own=a, nm=a, n=9, o=a: lib.dcv_eval_manifold_reduce(c, m, own, nm, n, o, None)
    assert red(c=None) == EINVAL and red(m=None) == EINVAL and red(nm=None) == EINVAL and red(o=None) == EINVAL and red(own=a + 4) == EINVAL and red(o=a + 4) == EINVAL
    assert red(n=0) == EINVAL and red(n=2 ** 31) == EINVAL
    assert lib.dcv_launch_count() == n0

    # Python: anything that is not a (n, D) fp32 device tensor is refused; so is a metric whose inputs are missing, by name
    l0 = E.launches()
    for bad in (torch.zeros(9, 8), torch.zeros(9, 8, dtype=torch.float64), np.zeros((9, 8), dtype=F32)):
        with pytest.raises(native.NativeError):
            E.row_norms(bad)
        with pytest.raises(native.NativeError):
            E.knn_radii(bad, 3)
        with pytest.raises(native.NativeError):
            E.manifold_counts(bad, bad, None)
        with pytest.raises(native.NativeError):
            E.manifold_metrics(bad, bad)
    for bad_k in (0, 17, 2.0, True):
        with pytest.raises(ValueError):
            E.Evaluator(lambda x: (x, None), metrics=("pr",), pr_k=bad_k)
        with pytest.raises(ValueError):
            E.Evaluator(lambda x: (x, None), metrics=("dc",), dc_k=bad_k)
    with pytest.raises(ValueError):
        E.Evaluator(lambda x: (x, None), metrics=("pr", "prd"))
    for name in ("pr", "dc"):
        ev = E.Evaluator(lambda x: (x, None), metrics=(name,))
        assert ev.metrics == (name,)
        with pytest.raises(native.NativeError, match=f'"{name}"'):
            ev.evaluate(object(), object(), 50, 2)      # no real features: refused before the generators are touched
    ev = E.Evaluator(lambda x: (x, None), metrics=("pr",))
    ev.n_real_feats = 3                                  # k = 3 needs four
    with pytest.raises(native.NativeError, match='"pr"'):
        ev.evaluate(object(), object(), 50, 2)
    ev.n_real_feats = 4
    with pytest.raises(native.NativeError, match='"pr"'):
        ev.evaluate(object(), object(), 3, 2)           # and four generated samples
    assert E.launches() == l0 and lib.dcv_launch_count() == n0


# ---- the mirror ---------------------------------------------------------------------------------------------------------------------------------------------
def test_mirror_on_a_line_with_a_duplicate_and_a_tie():
    """Points on a line, k = 2.  Reals 0, 0, 1, 3, 6 (a duplicate: each 0 has the other as a neighbour at distance 0, so rA = (1, 1, 1, 9, 25)); fakes
    2, 2.5, 4, 11, 20.  The fake at 2 lies exactly on the surface of the real 1's ball (d2 = 1 = rA) and the fake at 11 on that of the real 6's (25 = rA), which is
    the only ball it is in: with < instead of <= the precision would be 3/5, not 4/5."""
    from dcvgan_amd import evaluation as E
    a = np.array([[0.0], [0.0], [1.0], [3.0], [6.0]], dtype=F32)
    b = np.array([[2.0], [2.5], [4.0], [11.0], [20.0]], dtype=F32)
    h = E.manifold_host(a, b, 2)
    assert np.array_equal(h["rad2_a"], [1.0, 1.0, 1.0, 9.0, 25.0]) and np.array_equal(h["rad2_b"], [4.0, 2.25, 4.0, 72.25, 256.0])
    assert np.array_equal(h["count_ba"], [3, 2, 2, 1, 0]) and np.array_equal(h["dmin2_ba"], [1.0, 0.25, 1.0, 25.0, 196.0])
    assert np.array_equal(h["count_ab"], [1, 1, 2, 4, 3]) and np.array_equal(h["dmin2_ab"], [4.0, 4.0, 1.0, 0.25, 4.0])
    assert (h["precision"], h["recall"], h["density"], h["coverage"]) == (4 / 5, 1.0, 8 / (2 * 5), 3 / 5)
    same(h, brute(a, b, 2))
    assert ties(a, b, 2) >= 2
    assert np.array_equal((E.d2_host(b, a) < h["rad2_a"][None, :]).sum(axis=1), [2, 2, 2, 0, 0])      # what < would count


@pytest.mark.parametrize("na,nb,D,k", [(12, 9, 3, 3), (20, 17, 5, 5), (6, 6, 1, 5), (4, 4, 1, 3), (17, 2, 5, 1)])
def test_mirror_against_brute_force_on_integer_features(na, nb, D, k):
    from dcvgan_amd import evaluation as E
    a, b = integer_case(1000 + na + D, na, nb, D)
    h = E.manifold_host(a, b, k)
    same(h, brute(a, b, k))
    assert h["rad2_a"].dtype == F64 and h["count_ba"].dtype == np.int32


def test_mirror_refusals_and_non_finite_features():
    from dcvgan_amd import evaluation as E
    a, b = integer_case(5, 9, 8, 4)
    for bad in (0, 17):
        with pytest.raises(ValueError):
            E.manifold_host(a, b, bad)
    with pytest.raises(ValueError):
        E.manifold_host(a[:3], b, 3)                     # n < k + 1
    with pytest.raises(ValueError):
        E.manifold_host(a, b[:, :3], 3)
    a2 = a.copy()
    a2[4, 1] = np.nan
    h = E.manifold_host(a2, b, 3)
    assert all(np.isnan(h[key]) for key in ("precision", "recall", "density", "coverage"))
    keep = np.arange(9) != 4
    assert np.array_equal(h["rad2_a"][keep], E.knn_radii_host(a[keep], 3)) and h["rad2_a"][4] == np.inf      # the NaN row is nobody's neighbour and has none
    assert h["count_ba"].max() <= 8 and np.array_equal(h["dmin2_ba"], E.counts_host(b, a[keep], None)[1])
