"""GPU: the device-resident dataset (dcvgan_amd/clipstore.py, csrc/clipstore.hip).  The draw is held to the host mirror integer for integer, the gather
to dataprep.decode_* on frames the host gathered with the same table, byte for byte (np.array_equal everywhere: no tolerance), and the whole route to what the
reference's own VideoDataset.__getitem__ returned (tests/golden/dataset_norm.npz)."""
import math
import os

import numpy as np
import pytest
import torch

from tests import rig

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
MODES = {"colour+depth": ("depth", False), "flow": ("optical-flow", False), "segmentation": ("segmentation", False), "surreal-depth": ("depth", True)}


def _cs():
    from dcvgan_amd import clipstore, native
    native.lib()
    return clipstore


def _geo_frames(rng, n, H, W, info, surreal, kind=0):
    if info == "depth" and surreal:
        d = np.full((n, H, W), 1e10, dtype=np.float32)
        ys, xs = slice(H // 4, max(H // 4 + 1, 3 * H // 4)), slice(W // 4, max(W // 4 + 1, 3 * W // 4))
        shape = d[:, ys, xs].shape
        if kind == 0:      # a person
            d[:, ys, xs] = rng.uniform(2.0, 6.0, size=shape).astype(np.float32)
        elif kind == 1:    # a flat foreground: max == min
            d[:, ys, xs] = 3.5
        elif kind == 3:    # the foreground's range moves with time: every window has its own min and max
            d[:, ys, xs] = (rng.uniform(0.0, 0.5, size=shape) + 2.0 + np.arange(n)[:, None, None]).astype(np.float32)
        return d           # kind 2: no foreground
    if info == "depth":
        return rng.integers(0, 256, size=(n, H, W, 1), dtype=np.uint8)
    if info == "optical-flow":
        return (rng.standard_normal((n, H, W, 2)) * 9).astype(np.float32)
    return rng.integers(0, 25, size=(n, H, W), dtype=np.uint8)


def _videos(rng, counts, H, W, info, surreal):
    return [(rng.integers(0, 256, size=(n, H, W, 3), dtype=np.uint8), _geo_frames(rng, n, H, W, info, surreal, kind=i % 4)) for i, n in enumerate(counts)]


def _decode_on_host_gather(videos, table, T, info, surreal, image_size):
    """The existing path: the host cuts the table's windows and stacks them, dataprep.decode_* normalises the batch."""
    from dcvgan_amd import dataprep
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    color = np.stack([videos[c][0][t0:t0 + T] for c, t0 in table])
    geo = np.stack([videos[c][1][t0:t0 + T] for c, t0 in table])
    xc = dataprep.decode_color(up(color))
    if info == "depth" and surreal:
        xg = dataprep.decode_surreal_depth(up(geo))
    elif info == "depth":
        xg = dataprep.decode_depth(up(geo))
    elif info == "optical-flow":
        xg = dataprep.decode_flow(up(geo), image_size)
    else:
        xg = dataprep.decode_segmentation(up(geo), 25)
    return xc.cpu().numpy(), xg.cpu().numpy()


# ---- the draw -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 3, 17, 1000])
@pytest.mark.parametrize("B", [1, 5])
def test_draw_is_the_mirror(N, B):
    CS = _cs()
    T = 16
    counts = np.random.default_rng(N).choice([T, T + 1, T + 2, 300], size=N).tolist()
    st = CS.ClipStore(T, "depth", DEV).allocate(counts, 1, 1)
    if N < B:
        with pytest.raises(ValueError):
            CS.ClipSampler(st, B, seed=5, rank=0, world=1)
        return
    for rank, world in ((0, 1), (1, 2)) if N >= 2 * B else ((0, 1),):
        s = CS.ClipSampler(st, B, seed=5, rank=rank, world=world)
        seen = []
        for it, epoch in ((0, 0), (len(s) - 1, 0), (0, 1), (len(s) - 1, 3)):      # the first and the last batch of an epoch, the first of the next, a later one
            s.epoch, s.iteration = epoch, it
            got = s.draw().cpu().numpy()
            want = s.table_host()
            assert got.dtype == np.int32 and got.shape == (B, 2) and np.array_equal(got, want), (N, B, rank, epoch, it, got, want)
            n = np.asarray(counts)[got[:, 0]]
            assert np.all(got[:, 1] >= 0) and np.all(got[:, 1] <= np.maximum(n - T - 1, 0))
            seen.append(got)
        s.epoch, s.iteration = 0, len(s) - 1
        s.advance()
        assert (s.epoch, s.iteration) == (1, 0)
        if N >= 17:
            assert not np.array_equal(seen[0], seen[2])


# ---- the gather against the existing path ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", sorted(MODES))
def test_gather_is_decode_of_the_same_frames(mode):
    """(5, 5) colour frames are 75 bytes each: a window starts on no 4-byte boundary (the smallest shape at which a vector load goes wrong), T * 25 pixels is no
    multiple of four for T = 1; (6, 10) windows start on 4-byte but not on 16-byte boundaries; (64, 64) is the training shape."""
    CS = _cs()
    info, surreal = MODES[mode]
    rng = np.random.default_rng(3)
    for T in (1, 16):
        counts = [T + 3, T + 2, T, T + 6, T + 1, T + 4]
        tables = [[(5, 4)], [(0, 0), (3, 6), (1, 1), (2, 0), (3, 0)]]      # the first video, the last video, t0 = 0 and t0 = n - T; B = 1 and 5
        for H, W in ((5, 5), (6, 10), (64, 64)):
            videos = _videos(rng, counts, H, W, info, surreal)
            st = CS.ClipStore.from_arrays(videos, T, info, DEV, surreal=surreal)
            assert st.nbytes == CS.ClipStore.bytes_for(counts, H, W, info, surreal)
            for table in tables:
                s = CS.ClipSampler(st, len(table), seed=0, rank=0, world=1)
                batch = s.next_batch(table=torch.tensor(table, dtype=torch.int32, device=DEV))
                assert sorted(batch) == sorted(["color", info])
                want_c, want_g = _decode_on_host_gather(videos, table, T, info, surreal, H)
                got_c, got_g = batch["color"].cpu().numpy(), batch[info].cpu().numpy()
                assert got_c.shape == (len(table), 3, T, H, W) and got_c.dtype == np.float32 and np.array_equal(got_c, want_c), (mode, T, H, W, len(table))
                assert got_g.shape == want_g.shape and got_g.dtype == np.float32 and np.array_equal(got_g, want_g), (mode, T, H, W, len(table))
                if surreal and len(table) == 5:
                    # rows 1 and 4 are two windows of the video whose foreground moves: each is normalised by its OWN min and max (dataset.py:136-149)
                    for b in (1, 4):
                        fg = got_g[b][got_g[b] < 1.0]
                        assert fg.min() == -1.0 and math.isclose(float(fg.max()), 0.8, rel_tol=1e-6)
                    assert np.all(got_g[3] == 1.0)                                  # no foreground
                    assert set(np.unique(got_g[2]).tolist()) == {1.0, float(np.float32(3.5) * np.float32(1.8) - np.float32(1.0))}      # flat foreground: max == min, not rescaled


def test_refusals_on_the_device():
    CS = _cs()
    from dcvgan_amd.native import NativeError
    T = 4
    st = CS.ClipStore.from_arrays(_videos(np.random.default_rng(0), [T, T + 2], 6, 6, "depth", False), T, "depth", DEV)
    s = CS.ClipSampler(st, 2, seed=0, rank=0, world=1)
    n0 = CS.launches()
    for rows in ([[0, 0], [2, 0]], [[0, 1], [1, 0]], [[1, 3], [1, 0]], [[-1, 0], [1, 0]]):
        with pytest.raises(ValueError, match="clip table row"):
            s.next_batch(table=torch.tensor(rows, dtype=torch.int32, device=DEV))
    for bad in (torch.zeros(2, 2, dtype=torch.int32), torch.zeros(2, 2, dtype=torch.int64, device=DEV), torch.zeros(3, 2, dtype=torch.int32, device=DEV),
                torch.zeros(2, 4, dtype=torch.int32, device=DEV)[:, :2]):
        with pytest.raises(NativeError, match="clip table"):
            s.next_batch(table=bad)
    assert CS.launches() == n0 and (s.epoch, s.iteration) == (0, 0)      # every refusal came before the first launch


# ---- against the reference's own dataset class ------------------------------------------------------------------------------------------------------------------
def test_against_the_reference_dataset_class():
    """Stores built from the fixture's *_in arrays, each with its last frame repeated once: n = T + 1, so t0 is always 0, as in the fixture's generator (which pins
    np.random.randint to 0); next_batch() then returns what VideoDataset.__getitem__ returned for the clip each row names."""
    from tests import goldenio as G
    CS = _cs()
    fx = G.load("dataset_norm.npz")
    T = 16
    plus1 = lambda a: np.concatenate([a, a[-1:]])
    n = 0

    def check(videos, info, surreal, outs_c, outs_g, seed):
        nonlocal n
        st = CS.ClipStore.from_arrays([(plus1(c), plus1(g)) for c, g in videos], T, info, DEV, surreal=surreal, image_size=64)
        s = CS.ClipSampler(st, len(videos), seed=seed, rank=0, world=1)
        for _ in range(2):      # two epochs: two shuffles of the same clips
            batch = s.next_batch()
            table = s.last_table.cpu().numpy()
            assert sorted(table[:, 0].tolist()) == list(range(len(videos))) and np.all(table[:, 1] == 0)
            got_c, got_g = batch["color"].cpu().numpy(), batch[info].cpu().numpy()
            for b, clip in enumerate(table[:, 0]):
                assert np.array_equal(got_c[b], outs_c[clip]) and np.array_equal(got_g[b], outs_g[clip]), (info, surreal, b, clip)
                n += 1
        assert s.epoch == 2

    check([(fx[f"mock/{i}/color_in"], fx[f"mock/{i}/depth_in"]) for i in range(3)], "depth", False,
          [fx[f"mock/{i}/color_out"] for i in range(3)], [fx[f"mock/{i}/depth_out"] for i in range(3)], 1)
    check([(fx["mock/0/color_in"], fx["mock/0/flow_in"])], "optical-flow", False, [fx["mock/0/color_out"]], [fx["mock/0/flow_out"]], 2)
    sc = fx["surreal/0/color_in"]      # the fixture holds one SURREAL colour clip; the four geometry cases share it
    check([(sc, fx[f"surreal/{i}/depth_in"]) for i in range(4)], "depth", True, [fx["surreal/0/color_out"]] * 4, [fx[f"surreal/{i}/depth_out"] for i in range(4)], 3)
    check([(sc, fx[f"surreal/{i}/segm_in"]) for i in range(4)], "segmentation", False, [fx["surreal/0/color_out"]] * 4, [fx[f"surreal/{i}/segm_out"] for i in range(4)], 4)
    assert n == 2 * (3 + 1 + 4 + 4)


# ---- 64-bit addressing --------------------------------------------------------------------------------------------------------------------------------------------
def test_a_window_past_4_gib():
    """A 349,600-frame 64 x 64 x 3 colour store is 4.3 GB; its last video, 17 frames, starts past byte 2^32.  Only that video is written."""
    from dcvgan_amd import dataprep
    CS = _cs()
    T, F, H, W = 16, 349_600, 64, 64
    assert (F - 17) * H * W * 3 > 2 ** 32
    color = torch.empty((F, H, W, 3), dtype=torch.uint8, device=DEV)
    depth = torch.empty((F, H, W, 1), dtype=torch.uint8, device=DEV)
    rng = np.random.default_rng(8)
    c17, d17 = rng.integers(0, 256, size=(17, H, W, 3), dtype=np.uint8), rng.integers(0, 256, size=(17, H, W, 1), dtype=np.uint8)
    color[F - 17:].copy_(torch.from_numpy(c17))
    depth[F - 17:].copy_(torch.from_numpy(d17))
    st = CS.ClipStore.from_packed(color, depth, [F - 17, 17], T, "depth")
    assert st.color.data_ptr() == color.data_ptr() and st.nbytes == F * H * W * 4 + 24
    s = CS.ClipSampler(st, 2, seed=0, rank=0, world=1)
    batch = s.next_batch(table=torch.tensor([[1, 0], [1, 1]], dtype=torch.int32, device=DEV))
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    assert torch.equal(batch["color"], dataprep.decode_color(up(np.stack([c17[0:16], c17[1:17]]))))
    assert torch.equal(batch["depth"], dataprep.decode_depth(up(np.stack([d17[0:16], d17[1:17]]))))


# ---- no host involvement --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("surreal", [False, True])
def test_three_launches_and_nothing_else(surreal):
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    from dcvgan_amd import native
    CS = _cs()
    T = 16
    counts = [T, T + 1, 40] * 7
    st = CS.ClipStore.from_arrays(_videos(np.random.default_rng(1), counts, 8, 8, "depth", surreal), T, "depth", DEV, surreal=surreal)
    s = CS.ClipSampler(st, 4, seed=3, rank=0, world=1)
    budget = 4 if surreal else 3      # one draw, one gather per stream, one more launch for SURREAL depth
    assert s.launches_per_batch == budget
    s.next_batch()
    torch.cuda.synchronize()
    n0, m0 = native.launch_count(), CS.launches()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        torch.cuda.set_sync_debug_mode("error")      # (inside the profiler's own start / stop, which synchronise)
        try:
            batches, tables = [], []
            for _ in range(3):
                batches.append(s.next_batch())
                tables.append(s.last_table)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
    assert native.launch_count() - n0 == CS.launches() - m0 == 3 * budget
    events = {e.key: e.count for e in prof.key_averages() if e.device_type == DeviceType.CUDA}
    print(f"\n[clipstore] device activity over three batches: { {k[:48]: n for k, n in events.items()} }")
    foreign = {k[:160]: n for k, n in events.items() if "clip_" not in k}      # a torch kernel, a copy in either direction, a memset
    assert not foreign, foreign
    assert sum(events.values()) == 3 * budget and sum(n for k, n in events.items() if "clip_draw_kernel" in k) == 3
    assert len({b["color"].data_ptr() for b in batches}) == 3 and len({t.data_ptr() for t in tables}) == 3 and tables[2] is s.last_table      # fresh tensors per call
    assert s.iteration == 4 and np.array_equal(tables[2].cpu().numpy(), s.table_host(0, 3))


# ---- from_processed_dir ----------------------------------------------------------------------------------------------------------------------------------------------
def test_from_processed_dir(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    CS = _cs()
    T, H, W = 16, 8, 8
    rng = np.random.default_rng(5)
    videos = _videos(rng, [17, 17, 17], H, W, "depth", False)
    with open(tmp_path / "list.txt", "w") as f:
        for i, (c, d) in enumerate(videos):
            f.write(f"v{i:02d} 17\n")
            for sub in ("color", "depth"):
                os.makedirs(tmp_path / f"v{i:02d}" / sub)
            for t in range(17):
                Image.fromarray(c[t]).save(tmp_path / f"v{i:02d}" / "color" / f"{t:03d}.png")
                Image.fromarray(d[t, :, :, 0]).save(tmp_path / f"v{i:02d}" / "depth" / f"{t:03d}.png")
    st = CS.ClipStore.from_processed_dir(tmp_path, "png", T, "depth", DEV)
    assert st.n_frames == [17, 17, 17] and (st.H, st.W) == (H, W)
    assert np.array_equal(st.color.cpu().numpy(), np.concatenate([c for c, _ in videos])) and np.array_equal(st.geo.cpu().numpy(), np.concatenate([d for _, d in videos]))
    assert CS.ClipStore.from_processed_dir(tmp_path, "png", T, "depth", DEV, number_limit=2).N == 2
    s = CS.ClipSampler(st, 3, seed=9, rank=0, world=1)
    batch = s.next_batch()
    want_c, want_g = _decode_on_host_gather(videos, s.last_table.cpu().numpy().tolist(), T, "depth", False, H)
    assert np.array_equal(batch["color"].cpu().numpy(), want_c) and np.array_equal(batch["depth"].cpu().numpy(), want_g)


# ---- end to end -------------------------------------------------------------------------------------------------------------------------------------------------------
def test_two_iterations_fed_by_the_sampler():
    """Two StepRunner.step calls at debug widths, B = 2, fed by the sampler: the losses are finite and are those of a run fed the same batches built on the host
    with decode_*."""
    from dcvgan_amd import trainer
    CS = _cs()
    cfg = rig.small_cfg()
    T = cfg.video_length
    counts = [T, T + 1, 40, T + 5, 33]
    videos = _videos(np.random.default_rng(6), counts, 64, 64, "depth", False)
    st = CS.ClipStore.from_arrays(videos, T, "depth", DEV)

    def run(feed):
        models, _ = rig.seeded_models(cfg, DEV, 21, 9)
        opts = trainer.build_optimizers(cfg, models)
        runner = trainer.StepRunner(cfg, models, opts, trainer.build_loss(cfg), sync_losses=True)
        return [runner.step(xc, xg, t) for (xc, xg), t in zip(feed, (3, 11))]

    sampler = trainer.build_clip_sampler(cfg, st, seed=13, rank=0, world=1)
    assert sampler.batchsize == 2 and len(sampler) == 2
    tables = [sampler.table_host(0, 0), sampler.table_host(0, 1)]

    def from_sampler():
        for _ in range(2):
            b = sampler.next_batch()
            yield b["color"], b["depth"]

    def from_host():
        for t in tables:
            xc, xg = _decode_on_host_gather(videos, t.tolist(), T, "depth", False, 64)
            yield torch.from_numpy(xc).to(DEV), torch.from_numpy(xg).to(DEV)

    got, want = run(from_sampler()), run(from_host())
    assert sampler.epoch == 1 and sampler.iteration == 0
    print(f"\n[clipstore end to end] losses {got}")
    for g, w in zip(got, want):
        assert all(math.isfinite(float(v)) for v in g.values()), g
        assert g == w, (g, w)
    assert got[0] != got[1]
