"""No GPU: the host mirror of dcv_clipstore_draw (clipstore.permute_host / windows_host / table_host: the specification tests/test_clipstore_gpu.py holds the
kernel to, integer for integer) and the host logic of ClipStore / ClipSampler — the drop_last length, the ranks' slices of an epoch, the three-integer state, and
the refusals, which all come before any launch and are therefore raised here on CPU tensors."""
import numpy as np
import pytest
import torch

from dcvgan_amd import clipstore as CS
from dcvgan_amd.native import NativeError

T = 16


def test_philox_known_answers():
    """Random123's known-answer vectors for Philox4x32-10: the host generator is the one dcv_common.h implements."""
    out = CS.philox4x32_10(0, 0, 0, 0, 0, 0)
    assert [int(v) for v in out] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    out = CS.philox4x32_10(0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF)
    assert [int(v) for v in out] == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    out = CS.philox4x32_10(0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344, 0xA4093822, 0x299F31D0)
    assert [int(v) for v in out] == [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]


@pytest.mark.parametrize("N", [1, 2, 3, 5, 16, 17, 1000, 65537])
def test_permutation_is_a_bijection(N):
    pos = np.arange(N)
    a = CS.permute_host(7, 0, pos, N)
    assert a.dtype == np.int64 and np.array_equal(np.sort(a), pos)
    assert np.array_equal(a, CS.permute_host(7, 0, pos, N))                                # reproducible
    assert np.array_equal(a[3:9], CS.permute_host(7, 0, pos[3:9], N))                      # any position on its own
    if N >= 16:
        assert not np.array_equal(a, CS.permute_host(7, 1, pos, N))                        # another epoch
        assert not np.array_equal(a, CS.permute_host(8, 0, pos, N))                        # another seed
        assert np.array_equal(np.sort(CS.permute_host(8, 5, pos, N)), pos)


def test_small_shuffles_differ_between_epochs_and_seeds():
    for N in (2, 3, 5):
        pos = np.arange(N)
        assert len({tuple(CS.permute_host(7, e, pos, N)) for e in range(64)}) > 1
        assert len({tuple(CS.permute_host(s, 0, pos, N)) for s in range(64)}) > 1


def test_shuffle_is_uniform():
    """N = 7, epochs 0..6999: each of the 49 (position, clip) counts within 1000 +- 150.  A uniform shuffle has sigma = sqrt(7000 * 1/7 * 6/7) = 29.3 per cell:
    the bound is 5 sigma."""
    clips = CS.permute_host(1234, np.arange(7000)[:, None], np.arange(7)[None, :], 7)
    assert np.array_equal(clips[5], CS.permute_host(1234, 5, np.arange(7), 7)) and np.array_equal(np.sort(clips, axis=1), np.tile(np.arange(7), (7000, 1)))
    counts = np.zeros((7, 7), dtype=np.int64)
    np.add.at(counts, (np.tile(np.arange(7), 7000), clips.reshape(-1)), 1)
    print(f"\n[clipstore] shuffle counts: min {counts.min()}, max {counts.max()}")
    assert counts.sum() == 49000 and np.all(np.abs(counts - 1000) <= 150), counts


def test_window_start_range():
    pos = np.arange(4000)
    for n in (T, T + 1, T + 2, T + 7, 400):
        t0 = CS.windows_host(3, 2, pos, np.full(4000, n), T)
        if n == T:
            assert np.all(t0 == 0)
        else:
            assert t0.min() >= 0 and t0.max() <= n - T - 1      # np.random.randint(n - T): the last window is never drawn
    assert CS.windows_host(3, 2, pos, np.full(4000, T + 7), T).max() == 6


def test_window_start_is_uniform():
    """n - T = 5 over 50,000 positions: every start within 5 sigma of 10,000, sigma = sqrt(50000 * 0.2 * 0.8) = 89.4."""
    t0 = CS.windows_host(99, 0, np.arange(50000), np.full(50000, T + 5), T)
    hist = np.bincount(t0, minlength=5)
    print(f"\n[clipstore] window starts: {hist.tolist()}")
    assert len(hist) == 5 and np.all(np.abs(hist - 10000) <= 5 * 89.443), hist


def _store(counts, H=4, W=4, geometric_info="depth", surreal=False):
    return CS.ClipStore(T, geometric_info, "cpu", surreal=surreal).allocate(counts, H, W)


@pytest.mark.parametrize("world", [1, 2, 4])
def test_ranks_slices_are_the_single_process_batch(world):
    rng = np.random.default_rng(0)
    counts = rng.choice([T, T + 1, 40], size=103).tolist()
    st, B = _store(counts), 5
    one = CS.ClipSampler(st, B * world, seed=11, rank=0, world=1)
    ranks = [CS.ClipSampler(st, B, seed=11, rank=r, world=world) for r in range(world)]
    assert len(one) == 103 // (B * world) and all(len(s) == len(one) for s in ranks)      # drop_last
    used = []
    for it in range(len(one)):
        want = one.table_host()
        got = np.concatenate([s.table_host() for s in ranks])
        assert got.dtype == np.int32 and np.array_equal(got, want)
        used += want[:, 0].tolist()
        for s in ranks + [one]:
            s.advance()
    assert len(set(used)) == len(used) == len(one) * B * world                             # no clip twice within an epoch
    assert all(s.epoch == 1 and s.iteration == 0 for s in ranks + [one])
    assert not np.array_equal(one.table_host(), one.table_host(epoch=0, iteration=0))      # the next epoch is another shuffle


def test_len_and_drop_last():
    st = _store([T] * 10)
    assert len(CS.ClipSampler(st, 3, seed=0, rank=0, world=1)) == 3
    assert len(CS.ClipSampler(st, 5, seed=0, rank=1, world=2)) == 1
    with pytest.raises(ValueError):
        CS.ClipSampler(st, 11, seed=0, rank=0, world=1)
    with pytest.raises(ValueError):
        CS.ClipSampler(st, 3, seed=0, rank=0, world=4)
    with pytest.raises(ValueError):
        CS.ClipSampler(st, 3, seed=0, rank=2, world=2)


def test_seed_follows_torch():
    st = _store([T + 3] * 20)
    s = CS.ClipSampler(st, 4, rank=0, world=1)
    before = torch.initial_seed()
    try:
        torch.manual_seed(5)
        a = s.table_host()
        assert s.seed == 5 and np.array_equal(a, CS.ClipSampler(st, 4, seed=5, rank=0, world=1).table_host())
        torch.manual_seed(6)
        assert not np.array_equal(a, s.table_host())
    finally:
        torch.manual_seed(before)


@pytest.mark.parametrize("stop", [3, 5])      # in the middle of an epoch of 5 iterations, and at its boundary
def test_state_dict_round_trip(stop):
    counts = np.random.default_rng(1).choice([T, T + 1, 90], size=23).tolist()
    st = _store(counts)
    a = CS.ClipSampler(st, 4, seed=21, rank=0, world=1)
    assert len(a) == 5
    want = []
    for _ in range(12):
        want.append(a.table_host())
        a.advance()
    b = CS.ClipSampler(st, 4, seed=21, rank=0, world=1)
    for _ in range(stop):
        b.advance()
    sd = b.state_dict()
    assert sd == dict(seed=21, epoch=stop // 5, iteration=stop % 5)
    c = CS.ClipSampler(st, 4, seed=999, rank=0, world=1)
    c.load_state_dict(sd)
    for k in range(stop, 12):
        assert np.array_equal(c.table_host(), want[k]), k
        c.advance()
    with pytest.raises(ValueError):
        c.load_state_dict(dict(seed=1, epoch=0, iteration=5))


def test_store_sizes_and_refusals():
    counts = [T, T + 1, 30]
    for info, surreal, per_pixel in (("depth", False, 4), ("depth", True, 7), ("optical-flow", False, 11), ("segmentation", False, 4)):
        st = _store(counts, 5, 6, info, surreal)
        assert st.N == 3 and st.n_total_frames == sum(counts) and st.starts.tolist() == [0, T, 2 * T + 1, 2 * T + 31]
        assert st.nbytes == CS.ClipStore.bytes_for(counts, 5, 6, info, surreal) == sum(counts) * 30 * per_pixel + 32
    with pytest.raises(ValueError):
        _store([T, T - 1])                                                    # a video shorter than video_length
    with pytest.raises(ValueError):
        _store([])
    with pytest.raises(ValueError):
        CS.ClipStore(T, "normals", "cpu")
    st = _store(counts, 5, 6)
    color, depth = np.zeros((T, 5, 6, 3), np.uint8), np.zeros((T, 5, 6, 1), np.uint8)
    st.put(0, color, depth)
    st.put(0, torch.from_numpy(color), depth[..., 0])                         # grey frames without their channel axis
    with pytest.raises(NativeError):
        st.put(0, color.astype(np.float32), depth)                            # wrong dtype
    with pytest.raises(NativeError):
        st.put(1, color, depth)                                               # video 1 has T + 1 frames
    with pytest.raises(NativeError):
        st.put(0, color.transpose(0, 3, 1, 2), depth)                         # channel-first is not the disk layout
    with pytest.raises(ValueError):
        st.put(3, color, depth)
    with pytest.raises(NativeError):
        CS.ClipStore.from_packed(torch.zeros(sum(counts), 5, 6, 3, dtype=torch.uint8), torch.zeros(sum(counts), 5, 6, dtype=torch.uint8), counts, T, "depth")
    with pytest.raises(NativeError):
        CS.ClipStore.from_packed(torch.zeros(sum(counts) - 1, 5, 6, 3, dtype=torch.uint8), torch.zeros(sum(counts) - 1, 5, 6, 1, dtype=torch.uint8), counts, T, "depth")


def test_nothing_runs_on_cpu_tensors():
    """There is no CPU fallback: a store in host memory, a host table, a table of another type or shape are refused, and so is a row that names no window."""
    counts = [T, T + 1, 30]
    st = _store(counts)
    s = CS.ClipSampler(st, 2, seed=0, rank=0, world=1)
    with pytest.raises(NativeError, match="GPU only"):
        s.next_batch()
    with pytest.raises(NativeError, match="GPU only"):
        s.draw()
    with pytest.raises(NativeError, match="GPU only"):
        st.gather(torch.zeros(2, 2, dtype=torch.int32))
    assert (s.epoch, s.iteration) == (0, 0) and s.last_table is None          # a refused call moves nothing
    for bad in (torch.zeros(2, 2, dtype=torch.int32), torch.zeros(2, 2, dtype=torch.int64), torch.zeros(2, 3, dtype=torch.int32), torch.zeros(3, 2, dtype=torch.int32),
                np.zeros((2, 2), np.int32)):
        with pytest.raises(NativeError, match="clip table"):
            st.require_table(bad, 2)
    CS.check_rows([[0, 0], [1, 1], [2, 14]], counts, T)
    for rows in ([[3, 0]], [[-1, 0]], [[0, 1]], [[1, 2]], [[2, 15]], [[2, -1]]):
        with pytest.raises(ValueError, match="clip table row 0"):
            CS.check_rows(rows, counts, T)
