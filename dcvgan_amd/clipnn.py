"""Nearest-training-clip search on the device-resident dataset: are the samples copies of training clips?

A ``ClipStore`` holds every decoded frame of the training set in HBM as raw uint8 in disk layout, so the exact nearest training WINDOW of a sample — over every
window of every video — is one integer GEMM against the store (csrc/clipnn.hip, v_mfma_i32_32x32x32_i8) followed by diagonal sums and a top-k.  Everything is
integers; ``nearest_host`` states the quantity in numpy and the kernels are held to it with ``np.array_equal``.

    d(q, v, s) = sum_{t < T} sum_{j < K} (int(q_t[j]) - int(c[starts[v] + s + t][j]))^2            K = H*W*C bytes per frame, T = store.video_length

Per query the k windows with the smallest (d, v, s) in lexicographic order; a query with exclusion index e >= 0 skips every window of video e; windows never cross
a video boundary; places beyond the admissible windows hold rows (-1, -1) and distance INT64_MAX.  Nothing here reads the device: results are device tensors, and
``summarise_host`` is the one documented host read (for logging, like ``aug.p()``).  The reference has no counterpart.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np
import torch

from . import clipstore
from .native import NativeError, check, dims5, lib, ptr, stream_ptr

K_MAX = 8
FRAME_BYTES_MAX = 65536        # a frame's dot of shifted bytes stays below 2^31: 128 * 128 * 65536 = 2^30
CHUNK_STEP = 64                # window starts per chunk come in multiples of the GEMM's 64-frame tile
INT64_MAX = np.iinfo(np.int64).max
# memorisation_report draws its real windows with the sampler's kernel under a seed of its own: this offset keeps them apart from a ClipSampler with the same seed
REPORT_SEED_OFFSET = 0x6A09E667F3BCC909
_M64 = 0xFFFFFFFFFFFFFFFF

_STATS = {"launches": 0}


def launches() -> int:
    """Kernel launches this module has issued so far, in this process.  A call's count depends on shapes and the workspace bound only (``launches_for``)."""
    return _STATS["launches"]


def _call(name: str, n_launches: int, *args):
    check(getattr(lib(), name)(*args), name)
    _STATS["launches"] += n_launches


# --------------------------------------------------------------------------- #
# the specification, in numpy
# --------------------------------------------------------------------------- #
def clips_to_frames_host(clips_u8) -> np.ndarray:
    """uint8 (n, C, T, H, W) -> (n, T, H*W*C): each frame's bytes in disk order (H, W, C)."""
    x = np.asarray(clips_u8)
    if x.dtype != np.uint8 or x.ndim != 5:
        raise ValueError(f"clips: expected uint8 (n, C, T, H, W), got {x.dtype}{x.shape}")
    n, c, t, h, w = x.shape
    return np.ascontiguousarray(x.transpose(0, 2, 3, 4, 1)).reshape(n, t, h * w * c)


def nearest_host(frames, n_frames_list: Sequence[int], queries_u8, T: int, k: int, exclude=None):
    """The quantity by brute force, in int64: ``frames`` uint8 (F, H, W, C) (a store stream in disk layout; (F, H, W) is read as C = 1), ``queries_u8`` uint8
    (n, C, T, H, W).  -> (rows int32 (n, k, 2), dist int64 (n, k))."""
    f = np.asarray(frames)
    if f.dtype != np.uint8 or f.ndim not in (3, 4):
        raise ValueError(f"nearest_host: frames uint8 (F, H, W, C), got {f.dtype}{f.shape}")
    f = f.reshape(f.shape[0], -1).astype(np.int64)
    q = clips_to_frames_host(queries_u8).astype(np.int64)
    T, k = int(T), int(k)
    counts = [int(c) for c in n_frames_list]
    if q.shape[1] != T or q.shape[2] != f.shape[1] or sum(counts) != f.shape[0] or not 1 <= k <= K_MAX:
        raise ValueError(f"nearest_host: {q.shape[1]} frames of {q.shape[2]} bytes per query against T {T}, {f.shape[1]} bytes per frame, {f.shape[0]} frames, k {k}")
    ex = np.full(len(q), -1, dtype=np.int64) if exclude is None else np.asarray(exclude, dtype=np.int64).reshape(len(q))
    rows = np.full((len(q), k, 2), -1, dtype=np.int32)
    dist = np.full((len(q), k), INT64_MAX, dtype=np.int64)
    for i in range(len(q)):
        found = []
        start = 0
        for v, n_v in enumerate(counts):
            if v != ex[i]:
                for s in range(n_v - T + 1):
                    d = f[start + s:start + s + T] - q[i]
                    found.append((int((d * d).sum()), v, s))
            start += n_v
        for j, (d, v, s) in enumerate(sorted(found)[:k]):
            rows[i, j], dist[i, j] = (v, s), d
    return rows, dist


def report_table_host(seed: int, n_real: int, n_frames_list: Sequence[int], T: int) -> np.ndarray:
    """The (n_real, 2) table of real windows memorisation_report draws: epoch e holds positions 0 .. N - 1 of the keyed shuffle, rows e*N .. e*N + N - 1."""
    N = len(n_frames_list)
    s = (int(seed) + REPORT_SEED_OFFSET) & _M64
    parts = [clipstore.table_host(s, e, np.arange(min(N, int(n_real) - e * N)), n_frames_list, T) for e in range((int(n_real) + N - 1) // N)]
    return np.concatenate(parts, axis=0)


def summarise_host(fake_dist, real_dist) -> dict:
    """A HOST READ, for logging: the nearest distances (column 0 of (n, k) tables, or 1-D) of the samples and of the real windows to their nearest OTHER video.
    -> fake_median, real_median, ratio = fake_median / real_median (inf when the real median is 0), threshold = the 1st percentile of the real distances
    (numpy's linear interpolation) and fraction_below = the share of samples strictly closer to a training window than that.  Places without a window
    (INT64_MAX) are left out; a side with nothing left gives nan."""
    def column(d):
        d = d.detach().cpu().numpy() if isinstance(d, torch.Tensor) else np.asarray(d)
        d = d.reshape(len(d), -1)[:, 0].astype(np.int64)
        return d[d != INT64_MAX].astype(np.float64)
    fake, real = column(fake_dist), column(real_dist)
    if fake.size == 0 or real.size == 0:
        return dict(fake_median=float("nan"), real_median=float("nan"), ratio=float("nan"), threshold=float("nan"), fraction_below=float("nan"))
    fm, rm, thr = float(np.median(fake)), float(np.median(real)), float(np.percentile(real, 1))
    return dict(fake_median=fm, real_median=rm, ratio=fm / rm if rm > 0 else float("inf"), threshold=thr, fraction_below=float((fake < thr).mean()))


# --------------------------------------------------------------------------- #
# the device side
# --------------------------------------------------------------------------- #
def _stream(store, stream: str):
    """-> (frames tensor, C) of a uint8 stream; every refusal that needs no device."""
    if stream not in ("colour", "geometry"):
        raise ValueError(f"clipnn: stream is 'colour' or 'geometry', got {stream!r}")
    if store.color is None:
        raise NativeError("ClipStore: empty (allocate() and put(), or one of the from_* constructors)")
    if stream == "geometry":
        if store.geo_mode != clipstore.U8 or store.geo_tail != (1,):
            what = "SURREAL depth in metres" if store.surreal else store.geometric_info
            raise NativeError(f"clipnn: the geometry stream of this store is {what} ({store.geo.dtype}): squared byte distance is defined for uint8 grey depth only")
        frames, c = store.geo, 1
    else:
        frames, c = store.color, 3
    if store.H * store.W * c > FRAME_BYTES_MAX:
        raise NativeError(f"clipnn: H*W*C = {store.H * store.W * c} bytes per frame, at most {FRAME_BYTES_MAX} (a frame's dot of shifted bytes must stay below 2^31)")
    if store.n_total_frames >= 2 ** 31:
        raise NativeError(f"clipnn: {store.n_total_frames} frames; fewer than 2^31")
    store._require_device()
    return frames, c


def _check_k(k):
    if not isinstance(k, int) or isinstance(k, bool) or not 1 <= k <= K_MAX:
        raise ValueError(f"clipnn: k in 1..{K_MAX}, got {k!r}")


def _require_on(t, store, what: str):
    if not isinstance(t, torch.Tensor):
        raise NativeError(f"{what}: expected a device tensor, got {type(t).__name__}")
    if not t.is_cuda:
        raise NativeError(f"{what}: expected a HIP device tensor, got {t.device} — the search runs on the GPU only (there is no CPU fallback)")
    if t.device != store.color.device:
        raise NativeError(f"{what}: on {t.device}, the store on {store.color.device}")


def chunk_plan(n: int, T: int, k: int, n_frames_total: int, max_workspace_bytes: int):
    """-> (chunk_frames, n_chunks, workspace bytes): the largest multiple of 64 window starts per chunk whose workspace fits the bound.  Host arithmetic only."""
    windows = int(n_frames_total) - int(T) + 1
    if windows < 1:
        raise ValueError(f"clipnn: {n_frames_total} frames hold no window of {T}")
    L = lib()

    def need(steps):
        b = L.dcv_clipnn_workspace_bytes(n, T, k, steps * CHUNK_STEP)
        if b == 0:
            raise NativeError(f"dcv_clipnn_workspace_bytes: {L.dcv_last_error().decode(errors='replace')}")
        return b
    hi = (windows + CHUNK_STEP - 1) // CHUNK_STEP
    if need(1) > int(max_workspace_bytes):
        raise NativeError(f"clipnn: max_workspace_bytes = {max_workspace_bytes} is too small for one chunk of {CHUNK_STEP} window starts of {n} queries "
                          f"({need(1)} bytes: min_workspace_bytes)")
    lo = 1      # need(lo) fits
    if need(hi) <= int(max_workspace_bytes):
        lo = hi
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if need(mid) <= int(max_workspace_bytes) else (lo, mid)
    cf = lo * CHUNK_STEP
    return cf, (windows + cf - 1) // cf, need(lo)


def min_workspace_bytes(store, n: int, k: int = 1) -> int:
    """The smallest max_workspace_bytes nearest_windows accepts for n queries."""
    return int(lib().dcv_clipnn_workspace_bytes(int(n), store.video_length, int(k), CHUNK_STEP))


def launches_for(store, n: int, k: int = 1, table_queries: bool = False, max_workspace_bytes: int = 1 << 30) -> int:
    """Launches of one nearest_windows call: one to pack forms (a) / (b), then three per chunk (GEMM, diagonal sums with the workgroups' k best, merge)."""
    return (0 if table_queries else 1) + 3 * chunk_plan(int(n), store.video_length, int(k), store.n_total_frames, max_workspace_bytes)[1]


def nearest_windows(store, queries: torch.Tensor, k: int = 1, stream: str = "colour", exclude=None, max_workspace_bytes: int = 1 << 30):
    """-> (rows int32 (n, k, 2) = (video, t0), dist int64 (n, k)), device tensors; rows[:, 0] is a table ``store.gather`` takes.

    ``queries``: (a) uint8 (n, C, T, H, W), any strides; (b) fp32 (n, C, T, H, W), any strides, converted with dcv_videos_to_uint8's arithmetic; (c) an int32
    (n, 2) table of store windows, read as raw bytes from the store (its rows are the caller's responsibility, as for gather; a row that names no window gets no
    neighbour).  ``exclude``: None, an int32 (n,) device tensor of video indices (-1: nothing), or "own" with form (c).  Every refusal comes before the first
    launch; no host read, no torch kernel."""
    _check_k(k)
    if isinstance(exclude, str) and exclude != "own":
        raise ValueError(f"clipnn: exclude is None, an int32 (n,) device tensor or 'own', got {exclude!r}")
    frames, c = _stream(store, stream)
    T, H, W = store.video_length, store.H, store.W
    _require_on(queries, store, "clipnn queries")
    table = None
    if queries.dtype == torch.int32:
        store.require_table(queries)
        table, n = queries, int(queries.shape[0])
    elif queries.dtype in (torch.uint8, torch.float32):
        if queries.dim() != 5 or tuple(queries.shape[1:]) != (c, T, H, W) or queries.shape[0] < 1:
            raise NativeError(f"clipnn queries: expected (n >= 1, {c}, {T}, {H}, {W}) for the {stream} stream, got {tuple(queries.shape)}")
        n = int(queries.shape[0])
    else:
        raise NativeError(f"clipnn queries: uint8 or float32 clips (n, C, T, H, W) or an int32 (n, 2) table, got {queries.dtype}")
    if n > 65535 or n * T >= 2 ** 24:
        raise NativeError(f"clipnn: at most 65535 queries and fewer than 2^24 query frames per call, got {n} x {T}")
    ex, ex_stride = None, 1
    if isinstance(exclude, str):
        if table is None:
            raise NativeError("clipnn: exclude='own' needs the queries as a table of store windows (form (c)): clips have no video of their own")
        ex, ex_stride = table, 2
    elif exclude is not None:
        _require_on(exclude, store, "clipnn exclude")
        if exclude.dtype != torch.int32 or tuple(exclude.shape) != (n,) or not exclude.is_contiguous():
            raise NativeError(f"clipnn exclude: expected a contiguous int32 ({n},) tensor, got {exclude.dtype}{tuple(exclude.shape)}")
        ex = exclude
    cf, n_chunks, ws_bytes = chunk_plan(n, T, k, store.n_total_frames, max_workspace_bytes)
    dev, s = store.color.device, stream_ptr()
    packed = None
    if table is None:
        packed = torch.empty((n, T, H * W * c), dtype=torch.uint8, device=dev)
        xd = dims5(queries)
        _call("dcv_clipnn_pack_queries", 1, ptr(queries), int(queries.dtype == torch.float32), C.byref(xd), ptr(packed), s)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    rows = torch.empty((n, k, 2), dtype=torch.int32, device=dev)
    dist = torch.empty((n, k), dtype=torch.int64, device=dev)
    for i in range(n_chunks):
        _call("dcv_clipnn_search", 3, ptr(frames), ptr(store.starts), store.N, store.n_total_frames, T, H, W, c, ptr(packed), ptr(table), n, ptr(ex), ex_stride, k,
              i * cf, cf, ptr(rows), ptr(dist), ptr(ws), ws_bytes, s)
    return rows, dist


def gather_u8(store, table: torch.Tensor, stream: str = "colour") -> torch.Tensor:
    """uint8 (n, C, T, H, W): the STORED bytes of the table's windows (``store.gather`` followed by a uint8 conversion goes through fp32 and is not guaranteed to
    return them).  One launch."""
    frames, c = _stream(store, stream)
    store.require_table(table)
    _require_on(table, store, "clip table")
    B, T, H, W = int(table.shape[0]), store.video_length, store.H, store.W
    if B > 65535:
        raise NativeError(f"clipnn.gather_u8: at most 65535 clips per call, got {B}")
    out = torch.empty((B, c, T, H, W), dtype=torch.uint8, device=store.color.device)
    _call("dcv_clipnn_gather_u8", 1, ptr(frames), ptr(table), ptr(store.starts), store.N, B, T, H, W, c, ptr(out), stream_ptr())
    return out


def neighbour_grid(store, fakes_u8: torch.Tensor, rows: torch.Tensor, grid_rows: int, grid_cols: int) -> torch.Tensor:
    """The (1, T, 3, grid_rows*H, 2*grid_cols*W) mosaic of dcv_video_grid_u8: the samples on the left, each sample's nearest training window (``rows``: an
    (n, 2) table, e.g. nearest_windows(...)[0][:, 0] made contiguous by the caller, or (n, k, 2) whose k = 1) on the right.  Colour stream.  Two launches."""
    from . import monitor
    _stream(store, "colour")
    if isinstance(rows, torch.Tensor) and rows.dim() == 3 and rows.shape[1] == 1:
        rows = rows.view(rows.shape[0], 2)      # (n, 1, 2) is the same memory as (n, 2)
    _require_on(fakes_u8, store, "neighbour_grid samples")
    if fakes_u8.dtype != torch.uint8 or fakes_u8.dim() != 5 or tuple(fakes_u8.shape[1:]) != (3, store.video_length, store.H, store.W) or not fakes_u8.is_contiguous():
        raise NativeError(f"neighbour_grid: samples as contiguous uint8 (n, 3, {store.video_length}, {store.H}, {store.W}), got {fakes_u8.dtype}{tuple(fakes_u8.shape)}")
    store.require_table(rows, int(fakes_u8.shape[0]))
    if int(grid_rows) * int(grid_cols) != int(fakes_u8.shape[0]):
        raise NativeError(f"neighbour_grid: {fakes_u8.shape[0]} clips do not fill a {grid_rows} x {grid_cols} grid")
    near = gather_u8(store, rows, "colour")
    out = monitor.video_grid_u8(fakes_u8, near, int(grid_rows), int(grid_cols))
    _STATS["launches"] += 1
    return out


def memorisation_report(store, fakes: torch.Tensor, n_real: int, seed: int, k: int = 1, stream: str = "colour", max_workspace_bytes: int = 1 << 30) -> dict:
    """Device tensors fake_rows, fake_dist (the samples' nearest training windows), real_table (n_real windows drawn with dcv_clipstore_draw under a seed and
    epochs of its own: no sampler's state is touched), real_rows, real_dist (their nearest windows in every OTHER video: exclude="own").  ``summarise_host`` turns the
    two distance tables into the figures a paper prints."""
    _check_k(k)
    n_real, N, T = int(n_real), store.N, store.video_length
    if n_real < 1:
        raise ValueError(f"memorisation_report: n_real >= 1, got {n_real}")
    _stream(store, stream)
    if N < 2:
        raise ValueError("memorisation_report: the nearest OTHER video needs a store of at least two videos")
    fake_rows, fake_dist = nearest_windows(store, fakes, k, stream, None, max_workspace_bytes)
    real_table = torch.empty((n_real, 2), dtype=torch.int32, device=store.color.device)
    key = (int(seed) + REPORT_SEED_OFFSET + clipstore.SEED_SALT) & _M64
    for e in range((n_real + N - 1) // N):
        b = min(N, n_real - e * N)
        _call("dcv_clipstore_draw", 1, C.c_void_p(real_table.data_ptr() + 8 * e * N), b, ptr(store.starts), N, T, key, e, 0, stream_ptr())
    real_rows, real_dist = nearest_windows(store, real_table, k, stream, "own", max_workspace_bytes)
    return dict(fake_rows=fake_rows, fake_dist=fake_dist, real_table=real_table, real_rows=real_rows, real_dist=real_dist)
