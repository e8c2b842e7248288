"""GPU: the nearest-training-clip search (dcvgan_amd/clipnn.py, csrc/clipnn.hip).  Everything is integers: rows and distances are held to the numpy
mirror clipnn.nearest_host with np.array_equal, on small stores built with ClipStore.from_arrays."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
I64MAX = np.iinfo(np.int64).max


def _nn():
    from dcvgan_amd import clipnn, native
    native.lib()
    return clipnn


class Rig:
    """A store of random bytes in [lo, hi) with a grey-depth geometry stream, and its frames on the host."""

    def __init__(self, seed, counts, H, W, T, lo=0, hi=256, videos=None):
        from dcvgan_amd import clipstore
        rng = np.random.default_rng(seed)
        self.counts, self.T, self.H, self.W = list(counts), T, H, W
        self.videos = videos if videos is not None else [(rng.integers(lo, hi, size=(n, H, W, 3), dtype=np.uint8),
                                                          rng.integers(lo, hi, size=(n, H, W, 1), dtype=np.uint8)) for n in counts]
        self.colour = np.concatenate([c for c, _ in self.videos])
        self.grey = np.concatenate([g for _, g in self.videos])
        self.starts = np.concatenate([[0], np.cumsum(self.counts)])
        self.store = clipstore.ClipStore.from_arrays(self.videos, T, "depth", DEV)

    def frames(self, stream):
        return self.colour if stream == "colour" else self.grey

    def window(self, v, s, stream="colour"):
        """(C, T, H, W) uint8: the bytes of window (v, s) in the layout of a query clip."""
        f = self.frames(stream)[self.starts[v] + s:self.starts[v] + s + self.T]
        return np.ascontiguousarray(f.transpose(3, 0, 1, 2))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _host(*ts):
    return tuple(t.cpu().numpy() for t in ts)


def _check(rig, queries_u8, k, stream="colour", exclude=None, **kw):
    NN = _nn()
    ex = None if exclude is None else _dev(np.asarray(exclude, dtype=np.int32))
    rows, dist = NN.nearest_windows(rig.store, _dev(queries_u8), k=k, stream=stream, exclude=ex, **kw)
    assert rows.dtype == torch.int32 and tuple(rows.shape) == (len(queries_u8), k, 2) and dist.dtype == torch.int64 and tuple(dist.shape) == (len(queries_u8), k)
    want_rows, want_dist = NN.nearest_host(rig.frames(stream), rig.counts, queries_u8, rig.T, k, exclude)
    rows, dist = _host(rows, dist)
    assert np.array_equal(dist, want_dist), (dist, want_dist)
    assert np.array_equal(rows, want_rows), (rows, want_rows)
    return rows, dist


@pytest.fixture(scope="module")
def nine():
    """9 videos of 16 .. 23 frames (172 in all: no multiple of any tile), 6 x 6 x 3 = 108 bytes per frame (a ragged last K step), T = 16."""
    return Rig(11, [16, 17, 18, 19, 20, 21, 22, 23, 16], 6, 6, 16)


@pytest.fixture(scope="module")
def dup():
    """8 x 8 x 3 = 192 bytes (whole K steps), T = 16; video 3 is a copy of video 1."""
    rng = np.random.default_rng(12)
    vids = [(rng.integers(0, 256, size=(n, 8, 8, 3), dtype=np.uint8), rng.integers(0, 256, size=(n, 8, 8, 1), dtype=np.uint8)) for n in (16, 20, 23)]
    vids.append((vids[1][0].copy(), vids[1][1].copy()))
    return Rig(0, [16, 20, 23, 20], 8, 8, 16, videos=vids)


# ---- 1. against the mirror -------------------------------------------------------------------------------------------------------------------------------------------
CASES = {
    "whole-K-steps T2 n3 k3": dict(hwc=(8, 8, 3), T=2, n=3, k=3, counts=[2, 5, 10]),              # a video with n_v == T: one window; 17 frames
    "ragged-K T16 n17 k8": dict(hwc=(6, 6, 3), T=16, n=17, k=8, counts=[16, 17, 18, 19, 20, 21, 22, 23, 16]),      # ragged K, ragged frame count, two query tiles
    "geometry below-one-K-step T1 n1 k1": dict(hwc=(5, 7, 1), T=1, n=1, k=1, counts=[1, 3, 7]),
    "real-K T16 n3 k3": dict(hwc=(64, 64, 3), T=16, n=3, k=3, counts=[16, 17, 40]),
    "k beyond the windows": dict(hwc=(8, 8, 3), T=16, n=1, k=8, counts=[16, 17]),                  # 3 windows, k = 8: five places stay empty
    "geometry ragged-K T2 n17 k3": dict(hwc=(7, 9, 1), T=2, n=17, k=3, counts=[3, 2, 30, 36]),     # 63 bytes: one full and one part fragment per row
    "geometry no-whole-K-step T2 n3 k1": dict(hwc=(5, 5, 1), T=2, n=3, k=1, counts=[2, 4]),          # 25 bytes: fewer than the 32 of one MFMA
}


@pytest.mark.parametrize("name", list(CASES))
def test_against_the_mirror(name):
    c = CASES[name]
    H, W, C = c["hwc"]
    rig = Rig(1, c["counts"], H, W, c["T"])
    rng = np.random.default_rng(2)
    q = rng.integers(0, 256, size=(c["n"], C, c["T"], H, W), dtype=np.uint8)
    q[0] = rig.window(len(c["counts"]) - 1, 0, "colour" if C == 3 else "geometry")      # one query that is a window: distance 0
    rows, dist = _check(rig, q, c["k"], "colour" if C == 3 else "geometry")
    assert dist[0, 0] == 0 and rows[0, 0].tolist() == [len(c["counts"]) - 1, 0]
    if name == "k beyond the windows":
        assert (rows[0, 3:] == -1).all() and (dist[0, 3:] == I64MAX).all() and (rows[0, :3] >= 0).all()


# ---- 2. signedness and range -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q_byte,s_byte", [(255, 0), (0, 255), (128, 127), (127, 128)])
def test_signedness_and_range(q_byte, s_byte):
    NN = _nn()
    T, H, W = 16, 64, 64
    vids = [(np.full((n, H, W, 3), s_byte, dtype=np.uint8), np.zeros((n, H, W, 1), dtype=np.uint8)) for n in (16, 17)]
    rig = Rig(0, [16, 17], H, W, T, videos=vids)
    q = np.full((2, 3, T, H, W), q_byte, dtype=np.uint8)
    rows, dist = _host(*NN.nearest_windows(rig.store, _dev(q), k=3))
    d = (q_byte - s_byte) ** 2 * 12288 * 16
    assert d == (255 ** 2 if 255 in (q_byte, s_byte) else 1) * 12288 * 16
    assert np.array_equal(dist, np.full((2, 3), d, dtype=np.int64))
    assert np.array_equal(rows, np.array([[[0, 0], [1, 0], [1, 1]]] * 2, dtype=np.int32))      # all tied: (video, t0) order


# ---- 3. operand K order ----------------------------------------------------------------------------------------------------------------------------------------------
def test_operand_k_order_with_one_hot_frames():
    """Frames of 128 bytes (8 x 16 grey), T = 1.  Query j is nonzero only at byte j, store frame f only at byte f, with values that differ per byte and between
    the two sides (asymmetric): d(j, f) = q_j^2 + c_f^2 unless j == f, where it is (q_j - c_j)^2.  A fragment map that pairs byte j of one operand with another byte
    of the other — inside a K step (bytes 0 .. 63) or across steps (64 .. 127) — changes which pairs meet.  All 128 x 128 pairs are read back: 16 stores of 8
    frames, k = 8 (every window's distance is returned), and once against all 128 frames at k = 8."""
    NN = _nn()
    from dcvgan_amd import clipstore
    K = 128
    qv = np.array([1 + (7 * j) % 97 for j in range(K)], dtype=np.uint8)
    cv = np.array([200 - (11 * f) % 89 for f in range(K)], dtype=np.uint8)
    q = np.zeros((K, 1, 1, 8, 16), dtype=np.uint8)
    q.reshape(K, K)[np.arange(K), np.arange(K)] = qv
    grey = np.zeros((K, 8, 16, 1), dtype=np.uint8)
    grey.reshape(K, K)[np.arange(K), np.arange(K)] = cv
    colour = np.zeros((K, 8, 16, 3), dtype=np.uint8)
    qd = _dev(q)
    full = np.empty((K, K), dtype=np.int64)
    for g in range(16):
        st = clipstore.ClipStore.from_arrays([(colour[8 * g:8 * g + 8], grey[8 * g:8 * g + 8])], 1, "depth", DEV)
        rows, dist = _host(*NN.nearest_windows(st, qd, k=8, stream="geometry"))
        assert (rows[..., 0] == 0).all() and np.array_equal(np.sort(rows[..., 1], axis=1), np.tile(np.arange(8), (K, 1)))
        full[np.arange(K)[:, None], 8 * g + rows[..., 1]] = dist
    want = qv.astype(np.int64)[:, None] ** 2 + cv.astype(np.int64)[None, :] ** 2
    want[np.arange(K), np.arange(K)] = (qv.astype(np.int64) - cv.astype(np.int64)) ** 2
    assert np.array_equal(full, want)
    rig = Rig(0, [K], 8, 16, 1, videos=[(colour, grey)])
    _check(rig, q, 8, "geometry")


# ---- 4. planted neighbour, ties --------------------------------------------------------------------------------------------------------------------------------------
def test_planted_neighbour_and_the_tie_order(dup):
    q = np.stack([dup.window(1, 3), dup.window(2, 7), dup.window(0, 0)])
    b = int(q[0, 2, 5, 3, 4])
    q[0, 2, 5, 3, 4] = b + 5 if b < 250 else b - 5                                            # one byte moved by 5 (either way)
    q[1, 0, 15, 7, 7] ^= 0x80                                                                 # ... by 128
    rows, dist = _check(dup, q, 3)
    assert rows[0, :2].tolist() == [[1, 3], [3, 3]] and dist[0, :2].tolist() == [25, 25]      # video 3 repeats video 1: the lower index first
    assert rows[1, 0].tolist() == [2, 7] and dist[1, 0] == 128 ** 2
    assert rows[2, 0].tolist() == [0, 0] and dist[2, 0] == 0


# ---- 5. boundaries ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_a_window_across_two_videos_is_never_returned(nine):
    T = nine.T
    qs = []
    for a in (0, 3, 7):      # the last 8 frames of video a, then the first 8 of video a + 1: 16 consecutive frames of the packed buffer
        f = nine.colour[nine.starts[a + 1] - 8:nine.starts[a + 1] + 8]
        qs.append(f.transpose(3, 0, 1, 2))
    rows, dist = _check(nine, np.stack(qs), 8)
    assert (dist > 0).all()
    for i, a in enumerate((0, 3, 7)):
        for v, s in rows[i].tolist():
            assert 0 <= s <= nine.counts[v] - T


# ---- 6. exclude ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_exclude_tensor_and_own(nine):
    NN = _nn()
    from dcvgan_amd.native import NativeError
    q = np.stack([nine.window(2, 1), nine.window(5, 0), nine.window(8, 0), nine.window(0, 0)])
    rows, dist = _check(nine, q, 3, exclude=[2, -1, 8, -1])
    assert not (rows[0, :, 0] == 2).any() and not (rows[2, :, 0] == 8).any() and dist[0, 0] > 0 and dist[2, 0] > 0
    assert rows[1, 0].tolist() == [5, 0] and dist[1, 0] == 0 and rows[3, 0].tolist() == [0, 0] and dist[3, 0] == 0
    table = np.array([[2, 1], [5, 0], [8, 0], [0, 0], [7, 6]], dtype=np.int32)
    qt = np.stack([nine.window(v, s) for v, s in table])
    rows, dist = _host(*NN.nearest_windows(nine.store, _dev(table), k=3))
    assert np.array_equal(rows[:, 0], table) and (dist[:, 0] == 0).all()                       # without "own": the query itself comes first
    want = NN.nearest_host(nine.colour, nine.counts, qt, nine.T, 3)
    assert np.array_equal(rows, want[0]) and np.array_equal(dist, want[1])
    rows, dist = _host(*NN.nearest_windows(nine.store, _dev(table), k=3, exclude="own"))
    want = NN.nearest_host(nine.colour, nine.counts, qt, nine.T, 3, table[:, 0])
    assert np.array_equal(rows, want[0]) and np.array_equal(dist, want[1])
    assert not (rows[..., 0] == table[:, None, 0]).any() and (dist > 0).all()
    m0 = NN.launches()
    for bad in (_dev(q), _dev(q).float()):
        with pytest.raises(NativeError, match="own"):
            NN.nearest_windows(nine.store, bad, exclude="own")
    assert NN.launches() == m0


# ---- 7. query forms --------------------------------------------------------------------------------------------------------------------------------------------------
def test_query_forms_agree(nine):
    NN = _nn()
    from dcvgan_amd import sampling
    n, T, H, W = 5, nine.T, nine.H, nine.W
    rng = np.random.default_rng(3)
    frames = _dev((rng.standard_normal((n * T, 3, H, W)) * 0.8).astype(np.float32))      # the colour generator's memory: (B*T, C, H, W) ...
    videos = frames.view(n, T, 3, H, W).permute(0, 2, 1, 3, 4)                           # ... seen as (B, C, T, H, W): sample_videos' view
    assert not videos.is_contiguous()
    u8 = sampling._to_uint8(videos)                                                      # dcv_videos_to_uint8
    a = _host(*NN.nearest_windows(nine.store, u8, k=3))
    b = _host(*NN.nearest_windows(nine.store, videos, k=3))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    want = NN.nearest_host(nine.colour, nine.counts, u8.cpu().numpy(), T, 3)
    assert np.array_equal(a[0], want[0]) and np.array_equal(a[1], want[1])
    strided = _host(*NN.nearest_windows(nine.store, u8.permute(0, 2, 1, 3, 4).contiguous().permute(0, 2, 1, 3, 4), k=3))      # form (a) with other strides
    assert np.array_equal(a[0], strided[0]) and np.array_equal(a[1], strided[1])
    table = _dev(np.array([[1, 0], [4, 3], [8, 0]], dtype=np.int32))
    c = _host(*NN.nearest_windows(nine.store, table, k=3))
    ca = _host(*NN.nearest_windows(nine.store, NN.gather_u8(nine.store, table), k=3))
    assert np.array_equal(c[0], ca[0]) and np.array_equal(c[1], ca[1])
    # the grey stream, fp32 (n, 1, T, H, W)
    g = _dev((rng.standard_normal((2, 1, T, H, W)) * 0.8).astype(np.float32))
    ga = _host(*NN.nearest_windows(nine.store, g, k=2, stream="geometry"))
    want = NN.nearest_host(nine.grey, nine.counts, sampling._to_uint8(g).cpu().numpy(), T, 2)
    assert np.array_equal(ga[0], want[0]) and np.array_equal(ga[1], want[1])


def test_device_refusals_come_before_any_launch(nine):
    NN = _nn()
    from dcvgan_amd import native
    from dcvgan_amd.native import NativeError
    T, H, W = nine.T, nine.H, nine.W
    ok = torch.zeros((2, 3, T, H, W), dtype=torch.uint8, device=DEV)
    n0, m0 = native.launch_count(), NN.launches()
    for bad in (ok.cpu(), ok[:0], ok[:, :1], ok[:, :, :8], torch.zeros((2, 3, T, H, W + 1), dtype=torch.uint8, device=DEV), ok.to(torch.int16), ok.double(),
                torch.zeros((2, 3), dtype=torch.int32, device=DEV), torch.zeros((4, 2), dtype=torch.int32, device=DEV)[::2]):
        with pytest.raises(NativeError):
            NN.nearest_windows(nine.store, bad)
    with pytest.raises(NativeError, match="geometry"):
        NN.nearest_windows(nine.store, ok, stream="geometry")      # the grey stream has one channel
    for ex in (torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=torch.int64, device=DEV), torch.zeros(3, dtype=torch.int32, device=DEV)):
        with pytest.raises(NativeError, match="exclude"):
            NN.nearest_windows(nine.store, ok, exclude=ex)
    with pytest.raises(ValueError):
        NN.nearest_windows(nine.store, ok, k=9)
    assert native.launch_count() == n0 and NN.launches() == m0


# ---- 8. chunking -----------------------------------------------------------------------------------------------------------------------------------------------------
def test_chunking_changes_no_bit(nine):
    NN = _nn()
    from dcvgan_amd import native
    from dcvgan_amd.native import NativeError
    rng = np.random.default_rng(4)
    n, k = 17, 8
    q = rng.integers(0, 256, size=(n, 3, nine.T, nine.H, nine.W), dtype=np.uint8)
    q[3], q[16] = nine.window(0, 0), nine.window(8, 0)      # the first and the last window of the store
    least = NN.min_workspace_bytes(nine.store, n, k)
    assert NN.chunk_plan(n, nine.T, k, 172, least)[:2] == (64, 3) and NN.chunk_plan(n, nine.T, k, 172, 1 << 30)[1] == 1
    whole = _check(nine, q, k)
    parts = _check(nine, q, k, max_workspace_bytes=least)
    assert np.array_equal(whole[0], parts[0]) and np.array_equal(whole[1], parts[1])
    two = _check(nine, q, k, max_workspace_bytes=int(native.lib().dcv_clipnn_workspace_bytes(n, nine.T, k, 128)))
    assert np.array_equal(whole[0], two[0]) and np.array_equal(whole[1], two[1])
    table = _dev(np.array([[2, 1], [5, 0], [8, 0]], dtype=np.int32))
    t_whole = _host(*NN.nearest_windows(nine.store, table, k=k, exclude="own"))
    t_parts = _host(*NN.nearest_windows(nine.store, table, k=k, exclude="own", max_workspace_bytes=NN.min_workspace_bytes(nine.store, 3, k)))
    assert np.array_equal(t_whole[0], t_parts[0]) and np.array_equal(t_whole[1], t_parts[1])
    n0, m0 = native.launch_count(), NN.launches()
    with pytest.raises(NativeError, match="too small"):
        NN.nearest_windows(nine.store, _dev(q), k=k, max_workspace_bytes=least - 1)
    assert native.launch_count() == n0 and NN.launches() == m0


# ---- 9. - 11. the stored bytes, the figure, the table format ------------------------------------------------------------------------------------------------------------
def test_gather_u8_returns_the_stored_bytes(nine):
    NN = _nn()
    table = np.array([[0, 0], [8, 0], [7, 7], [3, 2], [3, 2]], dtype=np.int32)
    for stream in ("colour", "geometry"):
        out = NN.gather_u8(nine.store, _dev(table), stream)
        assert out.dtype == torch.uint8 and out.is_contiguous()
        assert np.array_equal(out.cpu().numpy(), np.stack([nine.window(v, s, stream) for v, s in table]))


def test_neighbour_grid_is_the_host_composition(nine):
    NN = _nn()
    from dcvgan_amd import monitor
    rng = np.random.default_rng(5)
    fakes = rng.integers(0, 256, size=(6, 3, nine.T, nine.H, nine.W), dtype=np.uint8)
    fakes[1], fakes[4] = nine.window(6, 2), nine.window(2, 0)
    fd = _dev(fakes)
    rows, _ = NN.nearest_windows(nine.store, fd, k=1)
    m0 = NN.launches()
    grid = NN.neighbour_grid(nine.store, fd, rows, 2, 3)
    assert NN.launches() - m0 == 2
    hr = rows.cpu().numpy()[:, 0]
    assert hr[1].tolist() == [6, 2] and hr[4].tolist() == [2, 0]
    near = np.stack([nine.window(v, s) for v, s in hr])
    assert np.array_equal(grid.cpu().numpy(), monitor.grid_host(fakes, near, 2, 3))


def test_rows_are_a_table_gather_takes(dup):
    NN = _nn()
    planted = np.array([[2, 7], [0, 0], [1, 4]], dtype=np.int32)
    q = np.stack([dup.window(v, s) for v, s in planted])
    rows, dist = NN.nearest_windows(dup.store, _dev(q), k=1)
    table = rows[:, 0]                                              # (n, 2) int32: k = 1 makes it contiguous as it is
    assert np.array_equal(table.cpu().numpy(), planted) and (dist.cpu().numpy() == 0).all()
    got_c, got_g = dup.store.gather(table)
    want_c, want_g = dup.store.gather(_dev(planted))
    assert torch.equal(got_c, want_c) and torch.equal(got_g, want_g)
    assert np.array_equal(NN.gather_u8(dup.store, table).cpu().numpy(), q)
    rows3, _ = NN.nearest_windows(dup.store, _dev(q), k=3)
    assert torch.equal(dup.store.gather(rows3[:, 0].contiguous())[0], want_c)
    r2, d2 = dup.store.nearest(_dev(q), k=1)                        # the forwarding method
    assert torch.equal(r2, rows) and torch.equal(d2, dist)


# ---- 12. - 13. repetition, launches -------------------------------------------------------------------------------------------------------------------------------------
def test_repetition_launch_count_and_nothing_else_on_the_device(nine):
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    from dcvgan_amd import native
    NN = _nn()
    rng = np.random.default_rng(6)
    n, k = 17, 3
    videos = _dev((rng.standard_normal((n * nine.T, 3, nine.H, nine.W)) * 0.8).astype(np.float32)).view(n, nine.T, 3, nine.H, nine.W).permute(0, 2, 1, 3, 4)
    ex = _dev(np.array([-1, 3] * 8 + [0], dtype=np.int32))
    table = _dev(np.array([[2, 1], [5, 0], [8, 0]], dtype=np.int32))
    small = NN.min_workspace_bytes(nine.store, n, k)
    first = NN.nearest_windows(nine.store, videos, k=k, exclude=ex, max_workspace_bytes=small)      # (also warms the allocator up)
    NN.nearest_windows(nine.store, videos, k=k, exclude=ex)
    NN.nearest_windows(nine.store, table, k=k, exclude="own")
    torch.cuda.synchronize()
    budget = [NN.launches_for(nine.store, n, k, max_workspace_bytes=small), NN.launches_for(nine.store, n, k), NN.launches_for(nine.store, 3, k, table_queries=True), 1]
    assert budget == [1 + 3 * 3, 1 + 3, 3, 1]
    n0, m0 = native.launch_count(), NN.launches()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        torch.cuda.set_sync_debug_mode("error")      # (inside the profiler's own start / stop, which synchronise)
        try:
            again = NN.nearest_windows(nine.store, videos, k=k, exclude=ex, max_workspace_bytes=small)
            whole = NN.nearest_windows(nine.store, videos, k=k, exclude=ex)
            own = NN.nearest_windows(nine.store, table, k=k, exclude="own")
            raw = NN.gather_u8(nine.store, table)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
    assert native.launch_count() - n0 == NN.launches() - m0 == sum(budget)
    events = {e.key: e.count for e in prof.key_averages() if e.device_type == DeviceType.CUDA}
    print(f"\n[clipnn] device activity: { {k_[:48]: c for k_, c in events.items()} }")
    foreign = {k_[:160]: c for k_, c in events.items() if "nn_" not in k_}      # a torch kernel, a copy in either direction, a memset
    assert not foreign, foreign
    assert sum(events.values()) == sum(budget) and sum(c for k_, c in events.items() if "nn_gemm_kernel" in k_) == 3 + 1 + 1
    for a, b in ((first, again), (first, whole)):      # two calls, and two chunkings: identical bits
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert raw.shape[0] == 3 and not (own[0][..., 0].cpu().numpy() == np.array([2, 5, 8])[:, None]).any()


# ---- 14. the report ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_memorisation_report_flags_exactly_the_copies():
    """6 distinct random videos of mid-range bytes [64, 192).  The fakes: 4 exact copies of store windows, 4 random clips of full-range bytes — per byte those lie
    an expected 5461 + 1365 (the two variances) from a store byte against 2 * 1365 between two store bytes, and over 3072 bytes a clip distance strays a few
    per cent from its expectation: every real-to-other-real distance is far below theirs."""
    NN = _nn()
    counts = [16, 18, 21, 17, 30, 19]
    rig = Rig(7, counts, 8, 8, 16, lo=64, hi=192)
    rng = np.random.default_rng(8)
    src = [(0, 0), (2, 5), (4, 14), (5, 3)]
    fakes = np.stack([rig.window(v, s) for v, s in src] + [rng.integers(0, 256, size=(3, 16, 8, 8), dtype=np.uint8) for _ in range(4)])
    order = [4, 0, 5, 1, 2, 6, 7, 3]                    # copies at places 1, 3, 4, 7
    fakes = fakes[order]
    is_copy = np.array([o < 4 for o in order])
    n_real = 15                                         # two and a half epochs of the draw
    m0 = NN.launches()
    rep = NN.memorisation_report(rig.store, _dev(fakes), n_real, seed=5, k=2)
    assert NN.launches() - m0 == (1 + 3) + 3 + 3
    assert sorted(rep) == ["fake_dist", "fake_rows", "real_dist", "real_rows", "real_table"] and all(t.is_cuda for t in rep.values())
    h = {name: t.cpu().numpy() for name, t in rep.items()}
    want = NN.nearest_host(rig.colour, counts, fakes, 16, 2)
    assert np.array_equal(h["fake_rows"], want[0]) and np.array_equal(h["fake_dist"], want[1])
    assert np.array_equal(h["fake_rows"][is_copy, 0], np.array([src[o] for o in order if o < 4], dtype=np.int32)) and (h["fake_dist"][is_copy, 0] == 0).all()
    assert (h["fake_dist"][~is_copy, 0] > 0).all()
    table = NN.report_table_host(5, n_real, counts, 16)
    assert np.array_equal(h["real_table"], table)
    want = NN.nearest_host(rig.colour, counts, np.stack([rig.window(v, s) for v, s in table]), 16, 2, table[:, 0])
    assert np.array_equal(h["real_rows"], want[0]) and np.array_equal(h["real_dist"], want[1])
    assert not (h["real_rows"][..., 0] == table[:, None, 0]).any()
    s = NN.summarise_host(rep["fake_dist"], rep["real_dist"])
    assert s["fraction_below"] == 0.5 and s["threshold"] > 0
    assert np.array_equal(h["fake_dist"][:, 0] < s["threshold"], is_copy)
    # another seed draws other windows; the sampler's state is no part of it
    assert not np.array_equal(NN.memorisation_report(rig.store, _dev(fakes), n_real, seed=6)["real_table"].cpu().numpy(), table)
