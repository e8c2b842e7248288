"""CPU: the nearest-training-clip search's specification and refusals (dcvgan_amd/clipnn.py).  nearest_host is held to a literal triple loop,
summarise_host to hand-made distances, and every refusal that needs no device is raised.  np.array_equal everywhere."""
import ctypes

import numpy as np
import pytest
import torch


def _nn():
    from dcvgan_amd import clipnn
    return clipnn


def _literal(frames, counts, queries, T, k, exclude):
    """d(q, v, s) written out index by index, then the k smallest (d, v, s)."""
    F, H, W, C = frames.shape
    n = queries.shape[0]
    rows = np.full((n, k, 2), -1, dtype=np.int32)
    dist = np.full((n, k), np.iinfo(np.int64).max, dtype=np.int64)
    starts = np.concatenate([[0], np.cumsum(counts)])
    for i in range(n):
        cand = []
        for v, n_v in enumerate(counts):
            if exclude is not None and exclude[i] == v:
                continue
            for s in range(n_v - T + 1):
                d = 0
                for t in range(T):
                    for y in range(H):
                        for x in range(W):
                            for c in range(C):
                                d += (int(queries[i, c, t, y, x]) - int(frames[starts[v] + s + t, y, x, c])) ** 2
                cand.append((d, v, s))
        cand.sort()
        for j, (d, v, s) in enumerate(cand[:k]):
            rows[i, j] = (v, s)
            dist[i, j] = d
    return rows, dist


def test_nearest_host_against_the_literal_loop():
    NN = _nn()
    rng = np.random.default_rng(0)
    T, H, W, C = 2, 2, 3, 3
    counts = [2, 4, 3]
    frames = rng.integers(0, 256, size=(sum(counts), H, W, C), dtype=np.uint8)
    frames[6:9] = frames[2:5]                       # video 2 repeats the first three frames of video 1: ties between (1, s) and (2, s)
    to_clip = lambda fr: np.ascontiguousarray(fr.transpose(3, 0, 1, 2))      # (T, H, W, C) -> (C, T, H, W)
    queries = np.stack([to_clip(frames[2:4]),       # window (1, 0) = window (2, 0): distance 0 twice, the lower video first
                        to_clip(frames[3:5]),       # (1, 1) = (2, 1)
                        to_clip(frames[1:3]),       # frames of videos 0 and 1: the window across the boundary does not exist
                        rng.integers(0, 256, size=(C, T, H, W), dtype=np.uint8)])
    for k, exclude in ((1, None), (3, None), (8, None), (3, [-1, 1, 0, 2]), (8, [1, 1, 1, 1])):
        rows, dist = NN.nearest_host(frames, counts, queries, T, k, exclude)
        want_rows, want_dist = _literal(frames, counts, queries, T, k, exclude)
        assert rows.dtype == np.int32 and dist.dtype == np.int64
        assert np.array_equal(rows, want_rows) and np.array_equal(dist, want_dist), (k, exclude)
    rows, dist = NN.nearest_host(frames, counts, queries, T, 8)
    assert rows[0, :2].tolist() == [[1, 0], [2, 0]] and dist[0, :2].tolist() == [0, 0]
    assert dist[2, 0] > 0                                                     # the boundary-crossing window was never a candidate
    assert (rows[:, 6:] == -1).all() and (dist[:, 6:] == np.iinfo(np.int64).max).all()      # 1 + 3 + 2 = 6 windows, k = 8
    rows, dist = NN.nearest_host(frames, counts, queries, T, 8, [1, 1, 1, 1])
    assert not (rows[..., 0] == 1).any() and (rows[:, 3:] == -1).all()
    # a (F, H, W) stream is C = 1
    grey = rng.integers(0, 256, size=(5, 2, 2), dtype=np.uint8)
    q = np.ascontiguousarray(grey[3:5][None, None])
    rows, dist = NN.nearest_host(grey, [5], q, 2, 1)
    assert rows.tolist() == [[[0, 3]]] and dist.tolist() == [[0]]
    with pytest.raises(ValueError):
        NN.nearest_host(frames, counts, queries, T, 9)
    with pytest.raises(ValueError):
        NN.nearest_host(frames, [2, 4], queries, T, 1)


def test_summarise_host_on_hand_made_distances():
    NN = _nn()
    real = np.arange(100, 201, dtype=np.int64)               # 101 values 100 .. 200: median 150, 1st percentile exactly 101
    fake = np.array([0, 100, 101, 150, 400], dtype=np.int64)
    s = NN.summarise_host(fake, real)
    assert s == dict(fake_median=101.0, real_median=150.0, ratio=101.0 / 150.0, threshold=101.0, fraction_below=2 / 5)
    # (n, k) tables: column 0 counts; places without a window are left out; tensors are read too
    big = np.iinfo(np.int64).max
    s2 = NN.summarise_host(torch.tensor([[0, 7], [100, 7], [101, 7], [150, 7], [400, 7], [big, big]]), np.stack([real, real + 5], axis=1))
    assert s2 == s
    assert NN.summarise_host(np.array([4, 4]), np.array([0, 0, 0]))["ratio"] == float("inf")
    assert np.isnan(NN.summarise_host(np.array([big]), real)["fake_median"])


def test_report_table_is_the_samplers_draw_under_another_seed():
    from dcvgan_amd import clipstore
    NN = _nn()
    counts = [16, 17, 40, 23, 16]
    t = NN.report_table_host(7, 12, counts, 16)
    assert t.shape == (12, 2) and t.dtype == np.int32
    for e, rows in enumerate((t[0:5], t[5:10], t[10:12])):
        assert np.array_equal(rows, clipstore.table_host((7 + NN.REPORT_SEED_OFFSET) & (2 ** 64 - 1), e, np.arange(len(rows)), counts, 16))
    assert sorted(t[:5, 0].tolist()) == [0, 1, 2, 3, 4]      # an epoch names every video once
    assert not np.array_equal(t[:5], clipstore.table_host(7, 0, np.arange(5), counts, 16))


def _cpu_store(H=4, W=4, T=2, info="depth", surreal=False, counts=(2, 3)):
    from dcvgan_amd import clipstore
    rng = np.random.default_rng(1)
    dtype, tail, _, _ = clipstore._geo_spec(info, surreal)
    vids = []
    for n in counts:
        geo = np.zeros((n, H, W) + tail, dtype=np.uint8 if dtype == torch.uint8 else np.float32)
        vids.append((rng.integers(0, 256, size=(n, H, W, 3), dtype=np.uint8), geo))
    return clipstore.ClipStore.from_arrays(vids, T, info, "cpu", surreal=surreal)


def test_refusals_that_need_no_device():
    from dcvgan_amd import clipstore
    from dcvgan_amd.native import NativeError
    NN = _nn()
    st = _cpu_store()
    q = torch.zeros((1, 3, 2, 4, 4), dtype=torch.uint8)
    for k in (0, 9, -1, 2.0, True):
        with pytest.raises(ValueError, match="k in 1..8"):
            NN.nearest_windows(st, q, k=k)
    with pytest.raises(ValueError, match="stream"):
        NN.nearest_windows(st, q, stream="flow")
    with pytest.raises(ValueError, match="exclude"):
        NN.nearest_windows(st, q, exclude="others")
    with pytest.raises(NativeError, match="empty"):
        NN.nearest_windows(clipstore.ClipStore(2, "depth", "cpu"), q)
    with pytest.raises(NativeError, match="empty"):
        NN.gather_u8(clipstore.ClipStore(2, "depth", "cpu"), torch.zeros((1, 2), dtype=torch.int32))
    # a CPU store (and with it CPU queries): the search runs on the GPU only
    with pytest.raises(NativeError, match="GPU only"):
        NN.nearest_windows(st, q)
    with pytest.raises(NativeError, match="GPU only"):
        st.nearest(q)
    with pytest.raises(NativeError, match="GPU only"):
        NN.memorisation_report(st, q, 4, 0)
    # the geometry stream is searched only where it is uint8 grey depth; every other store refuses it by name
    for info, surreal, name in (("optical-flow", False, "optical-flow"), ("segmentation", False, "segmentation"), ("depth", True, "SURREAL")):
        with pytest.raises(NativeError, match=name):
            NN.nearest_windows(_cpu_store(info=info, surreal=surreal), q, stream="geometry")
    # H*W*C > 65536: a frame's dot of shifted bytes could pass 2^31
    with pytest.raises(NativeError, match="65536"):
        NN.nearest_windows(_cpu_store(H=148, W=148, T=1, counts=(1,)), q)
    with pytest.raises(ValueError):
        NN.memorisation_report(st, q, 0, 0)
    with pytest.raises(ValueError, match="k in 1..8"):
        NN.memorisation_report(st, q, 4, 0, k=0)


def test_chunk_plan_is_host_arithmetic():
    from dcvgan_amd.native import NativeError
    NN = _nn()
    n, T, k, F = 17, 16, 8, 172
    least = NN.chunk_plan(n, T, k, F, 1 << 30)
    assert least[0] == 192 and least[1] == 1                       # 157 window starts, rounded up to the 64-frame tile: one chunk
    lo = int(NN.lib().dcv_clipnn_workspace_bytes(n, T, k, 64))
    assert NN.chunk_plan(n, T, k, F, lo) == (64, 3, lo)            # the smallest accepted bound: 64 window starts per chunk
    with pytest.raises(NativeError, match="too small"):
        NN.chunk_plan(n, T, k, F, lo - 1)
    mid = int(NN.lib().dcv_clipnn_workspace_bytes(n, T, k, 128))
    assert NN.chunk_plan(n, T, k, F, mid + 5)[:2] == (128, 2) and NN.chunk_plan(n, T, k, F, mid - 1)[:2] == (64, 3)
    with pytest.raises(ValueError):
        NN.chunk_plan(n, T, k, 15, 1 << 30)
    st = _cpu_store(counts=(2, 3))
    assert NN.launches_for(st, 3) == 1 + 3 and NN.launches_for(st, 3, table_queries=True) == 3
    assert NN.min_workspace_bytes(st, 3, 2) == int(NN.lib().dcv_clipnn_workspace_bytes(3, 2, 2, 64))


def test_c_entries_refuse_on_the_host():
    """Every DCV_EINVAL / DCV_EUNSUPPORTED / DCV_EWORKSPACE of the four entries is returned before any launch: none of these calls touches a device."""
    from dcvgan_amd import native
    from dcvgan_amd.native import Dims5
    L = native.lib()
    n0 = L.dcv_launch_count()
    for bad in ((0, 16, 1, 64), (65536, 16, 1, 64), (1, 0, 1, 64), (1, 4097, 1, 64), (65535, 4096, 1, 64), (1, 16, 0, 64), (1, 16, 9, 64), (1, 16, 1, 0), (1, 16, 1, 1 << 30)):
        assert L.dcv_clipnn_workspace_bytes(*bad) == 0 and b"clipnn_workspace_bytes" in L.dcv_last_error(), bad
    small, large = L.dcv_clipnn_workspace_bytes(2, 16, 3, 64), L.dcv_clipnn_workspace_bytes(2, 16, 3, 128)
    assert 2 * 16 * 128 * 4 <= small < large                      # 64 + 15 columns round up to 128
    buf = ctypes.create_string_buffer(4096)                       # never dereferenced
    p = (ctypes.addressof(buf) + 255) // 256 * 256
    xd = Dims5(1, 3, 2, 4, 4, 96, 32, 16, 4, 1)
    assert L.dcv_clipnn_pack_queries(None, 0, ctypes.byref(xd), p, None) == native.DCV_EINVAL
    assert L.dcv_clipnn_pack_queries(p, 2, ctypes.byref(xd), p, None) == native.DCV_EINVAL
    assert L.dcv_clipnn_pack_queries(p + 1, 1, ctypes.byref(xd), p, None) == native.DCV_EINVAL
    assert L.dcv_clipnn_pack_queries(p, 0, ctypes.byref(Dims5(1, 5, 2, 4, 4, 160, 32, 16, 4, 1)), p, None) == native.DCV_EINVAL
    assert L.dcv_clipnn_pack_queries(p, 0, ctypes.byref(Dims5(1, 3, 2, 148, 148, 0, 0, 0, 148, 1)), p, None) == native.DCV_EUNSUPPORTED
    ok = dict(frames=p, starts=p, N=2, F=40, T=16, H=4, W=4, C=3, queries=p, qtable=None, n=2, exclude=None, stride=1, k=3, c0=0, cf=64, rows=p, dist=p, ws=p, ws_bytes=small)

    def search(**kw):
        a = dict(ok, **kw)
        return L.dcv_clipnn_search(a["frames"], a["starts"], a["N"], a["F"], a["T"], a["H"], a["W"], a["C"], a["queries"], a["qtable"], a["n"], a["exclude"], a["stride"],
                                   a["k"], a["c0"], a["cf"], a["rows"], a["dist"], a["ws"], a["ws_bytes"], None)
    for kw in (dict(frames=None), dict(rows=None), dict(ws=None), dict(queries=None), dict(qtable=p), dict(starts=p + 4), dict(ws=p + 8), dict(exclude=p + 2),
               dict(C=0), dict(C=5), dict(N=0), dict(F=1 << 31), dict(F=15), dict(k=0), dict(k=9), dict(n=0), dict(T=0), dict(cf=0), dict(c0=-64), dict(c0=32), dict(c0=64),
               dict(exclude=p, stride=0)):
        assert search(**kw) == native.DCV_EINVAL, kw
        assert b"clipnn_search" in L.dcv_last_error(), kw
    assert search(H=148, W=148) == native.DCV_EUNSUPPORTED and b"65536" in L.dcv_last_error()
    assert search(ws_bytes=small - 1) == native.DCV_EWORKSPACE
    assert search(cf=128) == native.DCV_EWORKSPACE                # the workspace of 64 window starts does not hold 128
    g = dict(frames=p, table=p, starts=p, N=2, B=1, T=16, H=4, W=4, C=3, out=p)
    for kw in (dict(frames=None), dict(table=p + 2), dict(starts=p + 4), dict(out=None), dict(B=0), dict(B=65536), dict(T=0), dict(C=5), dict(N=0)):
        a = dict(g, **kw)
        assert L.dcv_clipnn_gather_u8(a["frames"], a["table"], a["starts"], a["N"], a["B"], a["T"], a["H"], a["W"], a["C"], a["out"], None) == native.DCV_EINVAL, kw
    assert L.dcv_launch_count() == n0
