"""CPU: PRD's binding, its refusals, the seeding's integer mirror, the curve and the numpy k-means mirror.

`prd_host` is the specification tests/test_prd_gpu.py holds the kernels to; here its parts are checked on inputs whose answers are known without it."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dcv_eval_prd_seed", "dcv_eval_prd_assign_workspace_bytes", "dcv_eval_prd_assign", "dcv_eval_prd_count", "dcv_eval_prd_update_workspace_bytes",
       "dcv_eval_prd_update")
F32, F64 = np.float32, np.float64


def blobs(seed, na, nb, D, C):
    """Integer blobs: K = max(2, C / 2) centres in [-12, 12]^D plus noise in [-2, 2], as fp32: every dot and every sum of rows is an exact integer in fp64."""
    g = np.random.default_rng(seed)
    K = max(2, C // 2)
    centres = g.integers(-12, 13, size=(K, D))
    a = centres[g.integers(0, K, size=na)] + g.integers(-2, 3, size=(na, D))
    b = centres[g.integers(0, K, size=nb)] + g.integers(-2, 3, size=(nb, D))
    return a.astype(F32), b.astype(F32)


@pytest.fixture(scope="module")
def lib():
    from dcvgan_amd import native
    if not os.path.exists(native.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return native.lib()


# ---- the binding --------------------------------------------------------------------------------------------------------------------------------------------
def test_new_names_are_bound_declared_and_exported(lib):
    from dcvgan_amd import evaluation as E, native
    header = open(os.path.join(ROOT, "include", "dcvgan_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    raw = ctypes.CDLL(native.LIB_PATH)
    for n in NEW:
        assert n in native.EXPORTS, n
        assert re.search(r"\b%s\s*\(" % n, code), f"{n} is not declared in dcvgan_hip.h"
        assert hasattr(raw, n), f"{n} is not exported by the library"
    for n in native.EXPORTS:
        assert re.search(r"\b%s\s*\(" % n, code), f"{n} is bound but not declared in dcvgan_hip.h"
    assert header.count("trainer.py:216-219") >= 5                             # every entry cites the call site
    m = re.search(r"#define\s+DCV_EVAL_PRD_SALT\s+0x([0-9A-Fa-f]+)ull", header)
    assert m and int(m.group(1), 16) == E.PRD_SALT and E.PRD_SALT != E.KID_SALT
    assert lib.dcv_version() == native.ABI_VERSION == 4
    assert re.search(r"for f in [^;]*\bevalprd\b", open(os.path.join(ROOT, "dcvgan_amd", "csrc", "build.sh")).read()), "csrc/evalprd.hip is not in build.sh's list"
    assert E.METRICS[:5] == ("is", "fid", "kid", "pr", "dc") and "prcurve" in E.METRICS and "prd" not in E.METRICS
    assert E.DEFAULT_METRICS == ("is", "fid", "kid")
    p = inspect.signature(E.Evaluator.__init__).parameters
    assert (p["prd_clusters"].default, p["prd_runs"].default, p["prd_iters"].default) == (20, 10, 20) and p["metrics"].default == ("is", "fid", "kid")
    p = inspect.signature(E.prd_kmeans).parameters
    assert [(k, v.default) for k, v in p.items()][2:] == [("num_clusters", 20), ("num_runs", 10), ("iters", 20), ("seed", 0), ("row_splits", 0)]
    assert inspect.signature(E.prd_update).parameters["row_splits"].default == 0
    assert inspect.signature(E.prd_curve).parameters["num_angles"].default == 1001 and inspect.signature(E.prd_f_beta).parameters["beta"].default == 8
    assert (E.prd_launches(20), E.prd_launches(0), E.prd_launches(8, with_norms=False)) == (106, 6, 44)
    assert "mini-batch" in E.prd_kmeans.__doc__ and "relocates" in E.prd_kmeans.__doc__ and "specification" in E.prd_curve.__doc__
    assert '"prd"' in E.Evaluator.__doc__ and "not attempted" not in E.__doc__


def test_refusals_need_no_gpu(lib):
    """The argument checks run on the host before any launch."""
    import torch
    from dcvgan_amd import evaluation as E, native
    buf = ctypes.create_string_buffer(256)      # never dereferenced
    a = (ctypes.addressof(buf) + 15) // 16 * 16
    n0, l0 = lib.dcv_launch_count(), E.launches()
    EINVAL, EWS = native.DCV_EINVAL, native.DCV_EWORKSPACE

    seed = lambda fa=a, sa=8, na=9, fb=a, sb=8, nb=7, D=8, C=5, R=2, c=a: lib.dcv_eval_prd_seed(fa, sa, na, fb, sb, nb, D, C, R, 0, c, None)
    assert seed(fa=None) == EINVAL and seed(fb=None) == EINVAL and seed(c=None) == EINVAL and seed(c=a + 4) == EINVAL
    assert seed(D=0) == EINVAL and seed(D=4097, sa=4097, sb=4097) == EINVAL and seed(sa=7) == EINVAL and seed(sb=7) == EINVAL and b"stride" in lib.dcv_last_error()
    assert seed(na=0) == EINVAL and seed(nb=0) == EINVAL and seed(na=2 ** 30, nb=2 ** 30) == EINVAL and b"2^31" in lib.dcv_last_error()
    assert seed(C=0) == EINVAL and seed(C=65, na=99) == EINVAL and seed(C=17) == EINVAL and b"C <= na + nb" in lib.dcv_last_error()      # 17 clusters, 16 rows
    assert seed(R=0) == EINVAL and seed(R=65) == EINVAL

    wa = lib.dcv_eval_prd_assign_workspace_bytes
    assert wa(20, 10) == 200 * 8 and wa(64, 64) == 4096 * 8 and wa(0, 1) == 0 and wa(65, 1) == 0 and wa(1, 0) == 0 and wa(1, 65) == 0
    asg = lambda fa=a, sa=8, na=9, fb=a, sb=8, nb=7, xa=a, xb=a, D=8, c=a, C=5, R=2, o=a, ws=a, wb=1 << 20: \
        lib.dcv_eval_prd_assign(fa, sa, na, fb, sb, nb, xa, xb, D, c, C, R, o, ws, wb, None)
    assert asg(fa=None) == EINVAL and asg(xa=None) == EINVAL and asg(xb=None) == EINVAL and asg(c=None) == EINVAL and asg(o=None) == EINVAL and asg(ws=None) == EINVAL
    assert asg(xa=a + 4) == EINVAL and asg(c=a + 4) == EINVAL and b"misaligned" in lib.dcv_last_error()
    assert asg(D=0) == EINVAL and asg(C=17) == EINVAL and asg(C=65, na=99) == EINVAL and asg(R=65) == EINVAL and asg(sa=7) == EINVAL
    assert asg(wb=10 * 8 - 1) == EWS and b"workspace" in lib.dcv_last_error()

    cnt = lambda o=a, xa=a, na=9, xb=a, nb=7, C=5, R=2, h=a: lib.dcv_eval_prd_count(o, xa, na, xb, nb, C, R, h, None)
    assert cnt(o=None) == EINVAL and cnt(xa=None) == EINVAL and cnt(xb=a + 4) == EINVAL and cnt(h=None) == EINVAL
    assert cnt(na=0) == EINVAL and cnt(nb=2 ** 31) == EINVAL and cnt(C=0) == EINVAL and cnt(C=65) == EINVAL and cnt(R=0) == EINVAL and cnt(R=65) == EINVAL

    # S * R * C * D * 8 bytes; S = row_splits, or for 0 max(1, min(64, ceil(n / 64), 1024 / (ceil(R C / 64) * ceil(D / 64))))
    wu = lib.dcv_eval_prd_update_workspace_bytes
    assert wu(135, 16, 20, 3, 2) == 2 * 60 * 16 * 8 and wu(135, 16, 20, 3, 64) == 64 * 60 * 16 * 8
    assert wu(135, 16, 20, 3, 0) == 3 * 60 * 16 * 8                           # one output tile, three row tiles
    assert wu(350, 64, 20, 10, 0) == 6 * 200 * 64 * 8                         # four output tiles, six row tiles
    assert wu(20000, 2048, 20, 10, 0) == 8 * 200 * 2048 * 8                   # 4 x 32 output tiles: 1024 / 128
    assert wu(20000, 4096, 64, 64, 0) == 1 * 4096 * 4096 * 8
    assert wu(0, 8, 5, 2, 0) == 0 and wu(2 ** 31, 8, 5, 2, 0) == 0 and wu(9, 0, 5, 2, 0) == 0 and wu(9, 4097, 5, 2, 0) == 0 and wu(9, 8, 65, 2, 0) == 0
    assert wu(9, 8, 5, 65, 0) == 0 and wu(9, 8, 5, 2, 65) == 0 and wu(9, 8, 5, 2, -1) == 0
    upd = lambda fa=a, sa=8, na=9, fb=a, sb=8, nb=7, xa=a, xb=a, o=a, D=8, C=5, R=2, S=0, c=a, h=a, ws=a, wb=1 << 20: \
        lib.dcv_eval_prd_update(fa, sa, na, fb, sb, nb, xa, xb, o, D, C, R, S, c, h, ws, wb, None)
    assert upd(fa=None) == EINVAL and upd(xa=None) == EINVAL and upd(o=None) == EINVAL and upd(c=None) == EINVAL and upd(h=None) == EINVAL and upd(ws=None) == EINVAL
    assert upd(c=a + 4) == EINVAL and upd(D=4097, sa=4097, sb=4097) == EINVAL and upd(C=17) == EINVAL and upd(R=0) == EINVAL and upd(sb=7) == EINVAL
    assert upd(S=-1) == EINVAL and upd(S=65) == EINVAL and b"row_splits" in lib.dcv_last_error()
    assert upd(wb=10 * 8 * 8 - 1) == EWS and upd(S=3, wb=3 * 10 * 8 * 8 - 1) == EWS and b"workspace" in lib.dcv_last_error()
    assert lib.dcv_launch_count() == n0

    # Python: anything that is not a (n, D) fp32 device tensor is refused
    for bad in (torch.zeros(9, 8), torch.zeros(9, 8, dtype=torch.float64), np.zeros((9, 8), dtype=F32)):
        for call in (lambda: E.prd_seed(bad, bad), lambda: E.prd_assign(bad, bad, torch.zeros(2, 5, 8, dtype=torch.float64)),
                     lambda: E.prd_update(bad, bad, torch.zeros(2, 18, dtype=torch.int32), torch.zeros(2, 5, 8, dtype=torch.float64)),
                     lambda: E.prd_kmeans(bad, bad), lambda: E.prd_metrics(bad, bad)):
            with pytest.raises(native.NativeError):
                call()
    with pytest.raises(native.NativeError):
        E.prd_count(torch.zeros(2, 18, dtype=torch.int32), torch.zeros(9, dtype=torch.float64), torch.zeros(9, dtype=torch.float64), 5)      # host tensors
    # the Evaluator: arguments out of range or of the wrong type, bool included; the reference's own name; missing inputs, by name
    for name in ("prd_clusters", "prd_runs", "prd_iters"):
        for bad in (-1, 65 if name != "prd_iters" else 1001, 2.0, True, "3", None):
            with pytest.raises(ValueError, match=name):
                E.Evaluator(lambda x: (x, None), metrics=("prcurve",), **{name: bad})
    for name in ("prd_clusters", "prd_runs"):
        with pytest.raises(ValueError, match=name):
            E.Evaluator(lambda x: (x, None), metrics=("prcurve",), **{name: 0})
    assert E.Evaluator(lambda x: (x, None), metrics=("prcurve",), prd_iters=0).prd_iters == 0
    with pytest.raises(ValueError):
        E.Evaluator(lambda x: (x, None), metrics=("prcurve", "prd"))
    ev = E.Evaluator(lambda x: (x, None), metrics=("prcurve",))
    assert ev.metrics == ("prcurve",) and ev._stores and (ev.prd_clusters, ev.prd_runs, ev.prd_iters) == (20, 10, 20)
    with pytest.raises(native.NativeError, match='"prcurve"'):
        ev.evaluate(object(), object(), 50, 2)          # no real features: refused before the generators are touched
    ev.n_real_feats = 9
    with pytest.raises(native.NativeError, match='"prcurve"'):
        ev.evaluate(object(), object(), 10, 2)          # 9 + 10 rows for 20 clusters
    ev = E.Evaluator(lambda x: (x, None), metrics=("prcurve",), max_features=5)
    ev.n_real_feats = 5
    with pytest.raises(native.NativeError, match='"prcurve"'):
        ev.evaluate(object(), object(), 50, 2)          # 5 + min(50, 5) rows for 20 clusters
    assert E.launches() == l0 and lib.dcv_launch_count() == n0


def test_mirror_refusals():
    from dcvgan_amd import evaluation as E
    a, b = blobs(1, 9, 7, 4, 5)
    for kw in (dict(num_clusters=0), dict(num_clusters=65), dict(num_clusters=17), dict(num_clusters=True), dict(num_clusters=5.0), dict(num_runs=0),
               dict(num_runs=65), dict(num_runs=True), dict(iters=-1), dict(iters=1001), dict(iters=2.5)):
        with pytest.raises(ValueError):
            E.prd_host(a, b, **{**dict(num_clusters=5, num_runs=2, iters=2), **kw})
    with pytest.raises(ValueError):
        E.prd_host(a, b[:, :3])
    for args in ((0, 0, 5, 9), (0, 65, 5, 9), (0, 2, 0, 9), (0, 2, 65, 99), (0, 2, 10, 9), (0, 2, 5, 2 ** 31)):
        with pytest.raises(ValueError):
            E.prd_seed_host(*args)
    with pytest.raises(ValueError):
        E.prd_curve(np.zeros((2, 3, 4), dtype=np.int32))
    with pytest.raises(ValueError):
        E.prd_curve(np.ones((2, 2, 4)))                  # counts are integers
    with pytest.raises(ValueError):
        E.prd_f_beta(np.ones(3), np.ones(4))
    with pytest.raises(ValueError):
        E.prd_f_beta(np.ones(3), np.ones(3), beta=0)


# ---- seeding ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,C,n", [(10, 20, 135), (2, 9, 9), (1, 1, 1)])
def test_seed_rows_are_distinct_per_run_and_repeatable(R, C, n):
    from dcvgan_amd import evaluation as E
    rows = E.prd_seed_host(7, R, C, n)
    assert rows.shape == (R, C) and rows.dtype == np.int32 and rows.min() >= 0 and rows.max() < n
    assert all(len(set(rows[r].tolist())) == C for r in range(R))
    assert np.array_equal(rows, E.prd_seed_host(7, R, C, n))
    if C == n:
        assert all(sorted(rows[r].tolist()) == list(range(n)) for r in range(R))      # a bijection
    if R > 1 and n > 9:
        assert not np.array_equal(rows[0], rows[1]) and not np.array_equal(rows, E.prd_seed_host(8, R, C, n))


def test_seed_is_the_kid_draws_bijection_under_its_own_key():
    """Run r's rows are what draw_host writes for subset r, side 0, had its key been seed + PRD_SALT: the same bijection, the run where the subset index goes."""
    from dcvgan_amd import evaluation as E
    n, R, C = 135, 4, 20
    shifted = (5 + E.PRD_SALT - E.KID_SALT) & E._M64     # draw_host adds KID_SALT to it
    assert np.array_equal(E.prd_seed_host(5, R, C, n), E.draw_host(shifted, R, C, n, n)[:, 0, :])


# ---- the curve ----------------------------------------------------------------------------------------------------------------------------------------------
def hist_of(real, fake, unassigned=(0, 0)):
    return np.array([[list(real) + [unassigned[0]], list(fake) + [unassigned[1]]]], dtype=np.int32)


def test_curve_of_equal_disjoint_and_half_covered_histograms():
    from dcvgan_amd import evaluation as E
    p, r = E.prd_curve(hist_of([3, 9, 1, 7], [3, 9, 1, 7]))
    assert p.shape == r.shape == (1001,) and p.dtype == F64
    assert abs(E.prd_f_beta(p, r, 8) - 1.0) <= 1e-9 and abs(E.prd_f_beta(p, r, 1 / 8) - 1.0) <= 1e-9
    p, r = E.prd_curve(hist_of([6, 14, 2, 0], [3, 7, 1, 0]))                   # unequal sizes: each side is normalised on its own
    assert abs(E.prd_f_beta(p, r) - 1.0) <= 1e-9
    p, r = E.prd_curve(hist_of([4, 6, 0, 0], [0, 0, 5, 5]))
    assert not p.any() and not r.any() and E.prd_f_beta(p, r, 8) == 0.0 and E.prd_f_beta(p, r, 1 / 8) == 0.0
    p, r = E.prd_curve(hist_of([5, 5], [10, 0]))                               # every fake is in a real cluster; half the reals are covered
    f8, f1_8 = E.prd_f_beta(p, r, 8), E.prd_f_beta(p, r, 1 / 8)
    print(f"\n[prd curve] fake [10, 0] vs real [5, 5]: max precision {p.max()}, max recall {r.max()}, F8 {f8:.4f}, F1/8 {f1_8:.4f}")
    assert p.max() == 1.0 and r.max() == 0.5 and f1_8 > f8 and abs(f1_8 - 0.985) < 1e-3 and abs(f8 - 0.504) < 1e-3
    assert (p >= 0).all() and (p <= 1).all() and (r >= 0).all() and (r <= 1).all()


def test_curve_swaps_with_the_sides_and_averages_the_runs():
    from dcvgan_amd import evaluation as E
    h = hist_of([5, 1, 7, 2], [2, 6, 3, 4])
    p, r = E.prd_curve(h)
    p2, r2 = E.prd_curve(h[:, ::-1])
    assert np.allclose(p2, r[::-1], rtol=0, atol=1e-9) and np.allclose(r2, p[::-1], rtol=0, atol=1e-9)      # slope -> 1 / slope: the angles are symmetric about pi / 4
    assert abs(E.prd_f_beta(p2, r2, 8) - E.prd_f_beta(r, p, 8)) <= 1e-9
    g = hist_of([5, 5, 3, 2], [10, 0, 1, 4])
    pa, ra = E.prd_curve(np.concatenate([h, g]))
    pg, rg = E.prd_curve(g)
    assert np.array_equal(pa, (p + pg) / 2) and np.array_equal(ra, (r + rg) / 2)


def test_an_unassigned_count_gives_nan():
    from dcvgan_amd import evaluation as E
    for un in ((1, 0), (0, 2)):
        h = np.concatenate([hist_of([5, 5], [6, 4]), hist_of([5, 4], [6, 4], un)])
        p, r = E.prd_curve(h)
        assert np.isnan(p).all() and np.isnan(r).all() and np.isnan(E.prd_f_beta(p, r, 8)) and np.isnan(E.prd_f_beta(p, r, 1 / 8))


# ---- the k-means mirror -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("na,nb,D,C,R", [(70, 65, 16, 20, 3), (33, 40, 7, 1, 1), (4, 4, 1, 3, 1)])
def test_mirror_on_integer_blobs_reaches_a_fixed_point(na, nb, D, C, R):
    from dcvgan_amd import evaluation as E
    a, b = blobs(na + D, na, nb, D, C)
    T = 8
    h = E.prd_host(a, b, C, R, T, seed=3)
    assert len(h["assign"]) == len(h["cent"]) == len(h["hist"]) == T + 1
    assert np.array_equal(h["cent"][0], np.concatenate([a, b]).astype(F64)[h["seed_rows"]])
    assert np.array_equal(h["assign"][-1], h["assign"][-2]) and np.array_equal(h["cent"][-1], h["cent"][-2])      # a fixed point before T
    for hist in h["hist"]:
        assert hist.dtype == np.int32 and hist.shape == (R, 2, C + 1)
        assert (hist[:, 0].sum(axis=1) == na).all() and (hist[:, 1].sum(axis=1) == nb).all() and not hist[:, :, C].any()
    x = np.concatenate([a, b]).astype(F64)
    for r in range(R):                                                         # the last centroids are the means of their rows; an empty cluster kept its own
        for c in range(C):
            rows = np.flatnonzero(h["assign"][-1][r] == c)
            if rows.size:
                assert np.allclose(h["cent"][-1][r, c], x[rows].mean(axis=0), rtol=1e-13, atol=0)
    assert 0.0 <= h["prd_f8"] <= 1.0 and 0.0 <= h["prd_f1_8"] <= 1.0
    # the assignment is the nearest centroid by explicit differences, the lowest index among exact ties
    c0 = h["cent"][0]
    for r in range(R):
        d2 = ((x[:, None, :] - c0[r][None, :, :]) ** 2).sum(axis=2)
        assert np.array_equal(h["assign"][0][r], d2.argmin(axis=1))


def test_mirror_keeps_an_empty_clusters_centroid_and_drops_a_non_finite_row():
    from dcvgan_amd import evaluation as E
    a = np.array([[0.0], [1.0], [2.0]], dtype=F32)
    b = np.array([[10.0], [11.0]], dtype=F32)
    cent = np.array([[[1.0], [1.0], [10.5], [100.0]]])                        # a duplicate (the lower index wins every row) and a far one: two empty clusters
    h = E.prd_host(a, b, 4, 1, 2, cent=cent)
    assert np.array_equal(h["assign"][0], [[0, 0, 0, 2, 2]])
    assert np.array_equal(h["cent"][1], [[[1.0], [1.0], [10.5], [100.0]]]) and np.array_equal(h["hist"][0], [[[3, 0, 0, 0, 0], [0, 0, 2, 0, 0]]])
    a[1, 0] = np.nan
    h = E.prd_host(a, b, 4, 1, 1, cent=cent)
    assert np.array_equal(h["assign"][0], [[0, 4, 0, 2, 2]]) and np.array_equal(h["hist"][-1], [[[2, 0, 0, 0, 1], [0, 0, 2, 0, 0]]])
    assert np.isnan(h["prd_f8"]) and np.isnan(h["prd_f1_8"]) and np.array_equal(h["cent"][1][0, :, 0], [1.0, 1.0, 10.5, 100.0])
