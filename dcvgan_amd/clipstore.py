"""The device-resident dataset: clips sampled and decoded on the GPU.

``StepRunner.step`` takes the real batch as a finished tensor, and the reference makes one with a DataLoader over ``VideoDataset`` (/root/reference/src/dataset.py:
111-186, train.py:101-109): 16 image reads per stream per clip, on the host, for every clip of every iteration.  The datasets are small next to the card — an
isogd-sized training set decodes to a few tens of GB — so a ``ClipStore`` keeps every video's decoded frames in HBM once, back to back in disk order, and a
``ClipSampler`` makes each batch there: one ``dcv_clipstore_draw`` launch writes a (B, 2) int32 table (clip, t0) — the epoch's shuffle, a stateless keyed bijection,
and the reference's random window — and one ``dcv_clipstore_gather`` launch per stream turns it into the normalised fp32 (B, C, T, H, W) batch with the arithmetic of
``dataprep.decode_*`` (SURREAL depth: one more launch).  No DataLoader, no worker, no PCIe traffic, no host read, no torch kernel.  The sampler's whole state is
(seed, epoch, iteration); data-parallel ranks read disjoint slices of the same epoch without talking to each other.

``permute_host`` / ``windows_host`` / ``table_host`` are an integer-exact numpy mirror of the draw: the specification the kernel is tested against, and what answers
"which clips were in iteration k" without a device.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import List, Optional, Sequence

import numpy as np
import torch

from .native import NativeError, check, lib, ptr, stream_ptr

U8, F32, LABELS = 0, 1, 2      # DCV_CLIP_U8 / _F32 / _LABELS
FEISTEL_ROUNDS = 8
NUM_SEGM_PARTS = 25            # dataset.py:177
# The draws' Philox key is the seed plus this constant: the models' latent draws and the augmentation's with the same seed run through other keys.
SEED_SALT = 0xD1B54A32D192ED03
_M64 = 0xFFFFFFFFFFFFFFFF

_STATS = {"launches": 0}


def launches() -> int:
    """Kernel launches this module has issued so far, in this process (every C entry it calls is one launch)."""
    return _STATS["launches"]


def _call(name: str, *args):
    check(getattr(lib(), name)(*args), name)
    _STATS["launches"] += 1


# --------------------------------------------------------------------------- #
# the host mirror of dcv_clipstore_draw (include/dcvgan_hip.h): integers only
# --------------------------------------------------------------------------- #
def philox4x32_10(c0, c1, c2, c3, k0: int, k1: int):
    """Philox4x32-10 (Salmon et al. 2011) on arrays of counters: four uint32 words in, four out (held in uint64 arrays)."""
    m = np.uint64(0xFFFFFFFF)
    c = [np.asarray(v, dtype=np.uint64) & m for v in (c0, c1, c2, c3)]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    s = np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> s) ^ c[1] ^ np.uint64(k0), p1 & m, (p0 >> s) ^ c[3] ^ np.uint64(k1), p0 & m]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c


def _key(seed: int):
    s = (int(seed) + SEED_SALT) & _M64
    return s & 0xFFFFFFFF, s >> 32


def half_bits(N: int) -> int:
    """h of the Feistel network on 2 h bits: the smallest even width that covers [0, N), at least 2."""
    bits = 0
    while (1 << bits) < N:
        bits += 1
    return max(2, bits + (bits & 1)) // 2


def permute_host(seed: int, epoch: int, positions, N: int) -> np.ndarray:
    """clip = perm(seed, epoch, position) for every position: the keyed bijection on [0, N) of dcv_clipstore_draw.  `epoch` is one epoch or an array that
    broadcasts against `positions`; the result is an int64 array of the broadcast shape."""
    N = int(N)
    pos, ep = np.broadcast_arrays(np.asarray(positions, dtype=np.int64), np.asarray(epoch, dtype=np.int64))
    if not 1 <= N < 2 ** 31 or (ep.size and ep.min() < 0):
        raise ValueError(f"permute_host: 1 <= N < 2^31 and epoch >= 0, got N {N}, epoch {epoch}")
    shape = pos.shape
    x, ep = pos.reshape(-1), ep.reshape(-1).astype(np.uint64)
    if x.size and (x.min() < 0 or x.max() >= N):
        raise ValueError(f"permute_host: positions must lie in [0, {N})")
    k0, k1 = _key(seed)
    e0, e1 = ep & np.uint64(0xFFFFFFFF), ep >> np.uint64(32)
    h = half_bits(N)
    mask = np.uint64((1 << h) - 1)
    x = x.astype(np.uint64)
    todo = np.ones(x.shape, dtype=bool)
    while todo.any():      # cycle walking: only the values still outside [0, N) go round again
        v = x[todo]
        L, R = v >> np.uint64(h), v & mask
        for r in range(FEISTEL_ROUNDS):
            f = philox4x32_10(R, r, e0[todo], e1[todo], k0, k1)[0] & mask
            L, R = R, L ^ f
        v = (L << np.uint64(h)) | R
        x[todo] = v
        todo[todo] = v >= np.uint64(N)
    return x.astype(np.int64).reshape(shape)


def windows_host(seed: int, epoch: int, positions, n_frames, T: int) -> np.ndarray:
    """t0 of the window at every position, whose clip has n_frames[i] frames: 0 if n <= T, else mulhi32(u, n - T) in [0, n - T - 1]."""
    pos = np.asarray(positions, dtype=np.int64)
    n = np.asarray(n_frames, dtype=np.int64)
    k0, k1 = _key(seed)
    epoch = int(epoch)
    u = philox4x32_10(pos.astype(np.uint64), 0xFFFFFFFF, epoch & 0xFFFFFFFF, (epoch >> 32) & 0xFFFFFFFF, k0, k1)[0]
    span = np.maximum(n - int(T), 0).astype(np.uint64)
    return ((u * span) >> np.uint64(32)).astype(np.int64)


def table_host(seed: int, epoch: int, positions, n_frames_list: Sequence[int], T: int) -> np.ndarray:
    """The (len(positions), 2) int32 table dcv_clipstore_draw writes for these positions of this epoch."""
    counts = np.asarray(n_frames_list, dtype=np.int64)
    clips = permute_host(seed, epoch, positions, len(counts))
    return np.stack([clips, windows_host(seed, epoch, positions, counts[clips], T)], axis=-1).astype(np.int32)


def check_rows(rows, n_frames_list: Sequence[int], T: int):
    """Refuse a table whose rows do not each name T frames of one video (ValueError)."""
    counts = np.asarray(n_frames_list, dtype=np.int64)
    for b, (clip, t0) in enumerate(np.asarray(rows, dtype=np.int64).reshape(-1, 2).tolist()):
        if not 0 <= clip < len(counts):
            raise ValueError(f"clip table row {b}: clip {clip} is not in [0, {len(counts)})")
        if t0 < 0 or t0 + int(T) > counts[clip]:
            raise ValueError(f"clip table row {b}: frames {t0} .. {t0 + int(T) - 1} are not inside video {clip} of {int(counts[clip])} frames")


# --------------------------------------------------------------------------- #
# the store
# --------------------------------------------------------------------------- #
def _geo_spec(geometric_info: str, surreal: bool):
    """-> (dtype, trailing shape of a frame after (H, W), gather mode, output channels) of the geometry stream in disk layout."""
    if geometric_info == "depth" and surreal:
        return torch.float32, (), F32, 1                   # depth.npy: metres, background 1e10 (dataset.py:134-156)
    if geometric_info == "depth":
        return torch.uint8, (1,), U8, 1                    # grey frames (dataset.py:157-166)
    if geometric_info == "optical-flow":
        return torch.float32, (2,), F32, 2                 # optical-flow.npy (dataset.py:168-174)
    if geometric_info == "segmentation":
        return torch.uint8, (), LABELS, NUM_SEGM_PARTS     # segm.npy (dataset.py:176-181)
    raise ValueError(f"ClipStore: unknown geometric_info {geometric_info!r}")


def _as_tensor(a, what: str, dtype, shape) -> torch.Tensor:
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    if t.dtype != dtype:
        raise NativeError(f"{what}: expected {dtype}, got {t.dtype}")
    if tuple(t.shape) != tuple(shape):
        raise NativeError(f"{what}: expected shape {tuple(shape)} (disk layout), got {tuple(t.shape)}")
    return t


class ClipStore:
    """``ClipStore(video_length, geometric_info, device, surreal=False)``: the decoded frames of a whole training set in device memory, in disk layout — colour uint8
    (F, H, W, 3); geometry uint8 (F, H, W, 1) grey depth, fp32 (F, H, W, 2) optical flow, uint8 (F, H, W) segmentation labels, or with ``surreal=True`` fp32 (F, H, W)
    depth in metres — F the frames of all videos back to back.  ``image_size`` (default: H) is what optical flow is divided by (dataset.py:174)."""

    def __init__(self, video_length: int, geometric_info: str, device, surreal: bool = False, image_size: Optional[int] = None):
        if int(video_length) < 1:
            raise ValueError(f"ClipStore: video_length >= 1, got {video_length}")
        self.video_length, self.geometric_info, self.device, self.surreal = int(video_length), geometric_info, torch.device(device), bool(surreal)
        self.geo_dtype, self.geo_tail, self.geo_mode, self.geo_channels = _geo_spec(geometric_info, self.surreal)
        self.image_size = image_size
        self.n_frames: List[int] = []
        self.starts_host: List[int] = [0]
        self.starts = self.color = self.geo = None
        self.H = self.W = 0

    # ---- construction --------------------------------------------------------------------------------------------------------------------------------------
    def _set_counts(self, n_frames_list, H: int, W: int):
        counts = [int(n) for n in n_frames_list]
        if not counts:
            raise ValueError("ClipStore: no videos")
        if len(counts) >= 2 ** 31:
            raise ValueError("ClipStore: fewer than 2^31 videos")
        for i, n in enumerate(counts):
            if n < self.video_length:
                raise ValueError(f"ClipStore: video {i} has {n} frames, fewer than video_length = {self.video_length}")
            if n >= 2 ** 31:
                raise ValueError(f"ClipStore: video {i} has {n} frames; fewer than 2^31")
        if int(H) < 1 or int(W) < 1:
            raise ValueError(f"ClipStore: H, W >= 1, got {H} x {W}")
        self.n_frames, self.H, self.W = counts, int(H), int(W)
        self.starts_host = [0]
        for n in counts:
            self.starts_host.append(self.starts_host[-1] + n)
        self.starts = torch.tensor(self.starts_host, dtype=torch.int64).to(self.device)      # a host tensor copied over once (no kernel)

    def allocate(self, n_frames_list: Sequence[int], H: int, W: int) -> "ClipStore":
        """Reserve the two packed buffers for videos of these frame counts (list.txt, dataset.py:86-97); fill them with put()."""
        self._set_counts(n_frames_list, H, W)
        F = self.starts_host[-1]
        self.color = torch.empty((F, self.H, self.W, 3), dtype=torch.uint8, device=self.device)
        self.geo = torch.empty((F, self.H, self.W) + self.geo_tail, dtype=self.geo_dtype, device=self.device)
        return self

    def put(self, i: int, color_u8, geo):
        """Copy video i's frames into place: host or device arrays in disk layout, colour (n, H, W, 3) uint8 and the geometry stream's (n, H, W[, C])."""
        if self.color is None:
            raise ValueError("ClipStore.put: allocate() first")
        if not 0 <= int(i) < self.N:
            raise ValueError(f"ClipStore.put: video {i} of {self.N}")
        n, a = self.n_frames[i], self.starts_host[i]
        if self.geo_tail == (1,) and getattr(geo, "ndim", 4) == 3:
            geo = geo[..., None]      # grey frames without their channel axis
        c = _as_tensor(color_u8, f"ClipStore.put: colour frames of video {i}", torch.uint8, (n, self.H, self.W, 3))
        g = _as_tensor(geo, f"ClipStore.put: {self.geometric_info} frames of video {i}", self.geo_dtype, (n, self.H, self.W) + self.geo_tail)
        self.color[a:a + n].copy_(c)
        self.geo[a:a + n].copy_(g)

    @classmethod
    def from_arrays(cls, videos, video_length: int, geometric_info: str, device, surreal: bool = False, image_size: Optional[int] = None) -> "ClipStore":
        """``videos``: a sequence of (colour, geometry) arrays in disk layout, one pair per video."""
        videos = list(videos)
        if not videos:
            raise ValueError("ClipStore: no videos")
        st = cls(video_length, geometric_info, device, surreal, image_size)
        st.allocate([len(c) for c, _ in videos], videos[0][0].shape[1], videos[0][0].shape[2])
        for i, (c, g) in enumerate(videos):
            st.put(i, c, g)
        return st

    @classmethod
    def from_packed(cls, color_dev: torch.Tensor, geo_dev: torch.Tensor, n_frames_list: Sequence[int], video_length: int, geometric_info: str,
                    surreal: bool = False, image_size: Optional[int] = None) -> "ClipStore":
        """Adopt two packed tensors that already exist (no copy): all videos' frames back to back, in the order of n_frames_list."""
        st = cls(video_length, geometric_info, color_dev.device, surreal, image_size)
        if color_dev.dim() != 4 or color_dev.shape[3] != 3:
            raise NativeError(f"ClipStore.from_packed: colour frames (F, H, W, 3), got {tuple(color_dev.shape)}")
        st._set_counts(n_frames_list, color_dev.shape[1], color_dev.shape[2])
        F = st.starts_host[-1]
        if geo_dev.device != color_dev.device:
            raise NativeError(f"ClipStore.from_packed: colour on {color_dev.device}, {geometric_info} on {geo_dev.device}")
        st.color = _as_tensor(color_dev, "ClipStore.from_packed: colour frames", torch.uint8, (F, st.H, st.W, 3))
        st.geo = _as_tensor(geo_dev, f"ClipStore.from_packed: {geometric_info} frames", st.geo_dtype, (F, st.H, st.W) + st.geo_tail)
        if not st.color.is_contiguous() or not st.geo.is_contiguous():
            raise NativeError("ClipStore.from_packed: the packed tensors must be contiguous")
        return st

    @classmethod
    def from_processed_dir(cls, root, ext: str, video_length: int, geometric_info: str, device, surreal: bool = False, number_limit: int = -1,
                           image_size: Optional[int] = None) -> "ClipStore":
        """Read the reference's processed layout (dataset.py:86-97, 125-181): ``list.txt`` with one "<folder> <n_frames>" line per video, ``<folder>/color/%03d.<ext>``
        and ``depth/%03d.<ext>`` (grey), ``optical-flow.npy``, ``segm.npy`` or, with surreal=True, ``depth.npy``.  Needs PIL for the images."""
        try:
            from PIL import Image
        except ImportError as e:
            raise NativeError("ClipStore.from_processed_dir reads the image files with PIL, which is not installed") from e
        root = str(root)
        with open(os.path.join(root, "list.txt")) as f:
            lines = [l.strip().split(" ") for l in f.readlines() if l.strip()]
        if number_limit != -1:
            lines = lines[:number_limit]
        if not lines:
            raise ValueError(f"ClipStore: {root}/list.txt names no video")
        paths, counts = [os.path.join(root, p) for p, _ in lines], [int(n) for _, n in lines]

        def image(path, grey):
            im = Image.open(path)
            return np.asarray(im.convert("L"), dtype=np.uint8)[..., None] if grey else np.asarray(im.convert("RGB"), dtype=np.uint8)

        st = cls(video_length, geometric_info, device, surreal, image_size)
        for i, (p, n) in enumerate(zip(paths, counts)):
            color = np.stack([image(os.path.join(p, "color", f"{t:03d}.{ext}"), False) for t in range(n)])
            if geometric_info == "depth" and surreal:
                geo = np.load(os.path.join(p, "depth.npy"), mmap_mode="r")[:n]
            elif geometric_info == "depth":
                geo = np.stack([image(os.path.join(p, "depth", f"{t:03d}.{ext}"), True) for t in range(n)])
            elif geometric_info == "optical-flow":
                geo = np.load(os.path.join(p, "optical-flow.npy"), mmap_mode="r")[:n]
            else:
                geo = np.load(os.path.join(p, "segm.npy"), mmap_mode="r")[:n]
            if i == 0:
                st.allocate(counts, color.shape[1], color.shape[2])
            st.put(i, color, np.ascontiguousarray(geo))
        return st

    # ---- what it holds -------------------------------------------------------------------------------------------------------------------------------------
    @property
    def N(self) -> int:
        return len(self.n_frames)

    @property
    def n_total_frames(self) -> int:
        return self.starts_host[-1]

    @staticmethod
    def bytes_for(n_frames_list: Sequence[int], H: int, W: int, geometric_info: str = "depth", surreal: bool = False) -> int:
        """Device bytes a store of these videos takes: both packed buffers and the prefix sum."""
        dtype, tail, _, _ = _geo_spec(geometric_info, surreal)
        per_pixel = 3 + torch.empty((), dtype=dtype).element_size() * int(np.prod(tail, dtype=np.int64))
        return int(sum(int(n) for n in n_frames_list)) * int(H) * int(W) * per_pixel + 8 * (len(n_frames_list) + 1)

    @property
    def nbytes(self) -> int:
        if self.color is None:
            return 0
        return self.color.numel() * self.color.element_size() + self.geo.numel() * self.geo.element_size() + self.starts.numel() * 8

    # ---- the gather ----------------------------------------------------------------------------------------------------------------------------------------
    def _require_device(self):
        if self.color is None:
            raise NativeError("ClipStore: empty (allocate() and put(), or one of the from_* constructors)")
        for t, what in ((self.color, "colour frames"), (self.geo, f"{self.geometric_info} frames"), (self.starts, "prefix sum")):
            if not t.is_cuda:
                raise NativeError(f"ClipStore: the {what} are on {t.device} — clips are gathered on the GPU only (there is no CPU fallback)")
            if t.device.index != torch.cuda.current_device():
                raise NativeError(f"ClipStore: the {what} are on {t.device} but the current device is cuda:{torch.cuda.current_device()}")

    def require_table(self, table: torch.Tensor, batch: Optional[int] = None):
        """Layout of a (B, 2) int32 device table; its rows are looked at by check_rows."""
        if not isinstance(table, torch.Tensor) or not table.is_cuda or table.dtype != torch.int32 or table.dim() != 2 or table.shape[1] != 2 \
                or table.shape[0] < 1 or (batch is not None and table.shape[0] != batch) or not table.is_contiguous():
            got = f"{table.dtype}{tuple(table.shape)} on {table.device}" if isinstance(table, torch.Tensor) else type(table).__name__
            raise NativeError(f"clip table: expected a contiguous ({batch if batch is not None else 'B'}, 2) int32 device tensor, got {got}")

    def gather(self, table: torch.Tensor):
        """(colour (B, 3, T, H, W), geometry (B, C, T, H, W)) of the table's windows: one launch per stream, one more for SURREAL depth.  The table's layout is
        checked here, its rows by the caller who made it (ClipSampler checks an injected table; a drawn one is right by construction)."""
        self._require_device()
        self.require_table(table)
        B, T, H, W = int(table.shape[0]), self.video_length, self.H, self.W
        if B > 65535:
            raise NativeError(f"ClipStore.gather: at most 65535 clips per batch, got {B}")
        color = torch.empty((B, 3, T, H, W), dtype=torch.float32, device=self.device)
        geo = torch.empty((B, self.geo_channels, T, H, W), dtype=torch.float32, device=self.device)
        s = stream_ptr()
        _call("dcv_clipstore_gather", ptr(self.color), U8, ptr(table), ptr(self.starts), self.N, B, T, H, W, 3, 127.5, 1.0, ptr(color), s)
        if self.geo_mode == LABELS:
            _call("dcv_clipstore_gather", ptr(self.geo), LABELS, ptr(table), ptr(self.starts), self.N, B, T, H, W, self.geo_channels, 1.0, 0.0, ptr(geo), s)
        elif self.surreal:
            _call("dcv_clipstore_gather", ptr(self.geo), F32, ptr(table), ptr(self.starts), self.N, B, T, H, W, 1, 1.0, 0.0, ptr(geo), s)      # x / 1 - 0: the raw window
            _call("dcv_clipstore_surreal", ptr(geo), B, T * H * W, s)
        elif self.geo_mode == F32:
            size = float(self.image_size if self.image_size is not None else H)
            _call("dcv_clipstore_gather", ptr(self.geo), F32, ptr(table), ptr(self.starts), self.N, B, T, H, W, self.geo_channels, size, 0.0, ptr(geo), s)
        else:
            _call("dcv_clipstore_gather", ptr(self.geo), U8, ptr(table), ptr(self.starts), self.N, B, T, H, W, 1, 127.5, 1.0, ptr(geo), s)
        return color, geo

    @property
    def launches_per_gather(self) -> int:
        return 3 if self.surreal else 2

    def nearest(self, queries: torch.Tensor, k: int = 1, stream: str = "colour", exclude=None, max_workspace_bytes: int = 1 << 30):
        """The k nearest training windows of every query clip, over every window of every video: clipnn.nearest_windows(self, ...)."""
        from . import clipnn
        return clipnn.nearest_windows(self, queries, k, stream, exclude, max_workspace_bytes)


# --------------------------------------------------------------------------- #
# the sampler
# --------------------------------------------------------------------------- #
class ClipSampler:
    """``ClipSampler(store, batchsize, seed=None, rank=None, world=None)``: the DataLoader of train.py:101-109 (shuffle=True, drop_last=True) over a ClipStore.

    ``for batch in sampler`` yields what is left of the current epoch as ``{"color": .., <geometric_info>: ..}`` dicts of device tensors (the keys of
    dataset.py:186, which trainer.py:293-296 reads) and ends with the epoch counter advanced; ``next_batch()`` makes one batch without the iterator.
    ``len(sampler) = N // (batchsize * world)``.  Row b of iteration i on rank r is epoch position (i * world + r) * batchsize + b, so the ranks' batches of an
    iteration, concatenated in rank order, are the batch a single process of batch size batchsize * world makes, and no clip is used twice in an epoch.
    Without ``seed`` the seed follows ``torch.initial_seed()``, as PhiloxRng's does; ``rank`` / ``world`` default to torch.distributed's when it is initialised,
    else 0 / 1.  ``last_table`` is the device table of the last batch; ``next_batch(table=...)`` injects one (tests).
    The state is (seed, epoch, iteration): ``state_dict()`` / ``load_state_dict()`` resume with the same batches, bit for bit."""

    def __init__(self, store: ClipStore, batchsize: int, seed: Optional[int] = None, rank: Optional[int] = None, world: Optional[int] = None):
        if rank is None or world is None:
            import torch.distributed as dist
            on = dist.is_available() and dist.is_initialized()
            rank = (dist.get_rank() if on else 0) if rank is None else rank
            world = (dist.get_world_size() if on else 1) if world is None else world
        self.store, self.batchsize, self.rank, self.world = store, int(batchsize), int(rank), int(world)
        if self.batchsize < 1 or self.world < 1 or not 0 <= self.rank < self.world:
            raise ValueError(f"ClipSampler: batchsize >= 1 and 0 <= rank < world, got batchsize {batchsize}, rank {rank}, world {world}")
        if len(self) == 0:
            raise ValueError(f"ClipSampler: {store.N} videos do not fill one batch of {self.batchsize} x {self.world} ranks (drop_last)")
        self._fixed_seed = None if seed is None else int(seed)
        self.epoch, self.iteration = 0, 0
        self.last_table: Optional[torch.Tensor] = None

    def __len__(self) -> int:
        return self.store.N // (self.batchsize * self.world)

    @property
    def seed(self) -> int:
        return (self._fixed_seed if self._fixed_seed is not None else torch.initial_seed()) & _M64

    def first_position(self, iteration: Optional[int] = None, rank: Optional[int] = None) -> int:
        i, r = self.iteration if iteration is None else int(iteration), self.rank if rank is None else int(rank)
        return (i * self.world + r) * self.batchsize

    def table_host(self, epoch: Optional[int] = None, iteration: Optional[int] = None, rank: Optional[int] = None) -> np.ndarray:
        """The table of (epoch, iteration) on `rank` (default: the batch next_batch() makes next on this rank), from the host mirror: no device involved."""
        p = self.first_position(iteration, rank)
        return table_host(self.seed, self.epoch if epoch is None else epoch, np.arange(p, p + self.batchsize), self.store.n_frames, self.store.video_length)

    def draw(self) -> torch.Tensor:
        """The table of the current (epoch, iteration): one launch; the state does not move."""
        st = self.store
        st._require_device()
        table = torch.empty((self.batchsize, 2), dtype=torch.int32, device=st.device)
        _call("dcv_clipstore_draw", ptr(table), self.batchsize, ptr(st.starts), st.N, st.video_length, (self.seed + SEED_SALT) & _M64, self.epoch,
              self.first_position(), stream_ptr())
        return table

    def next_batch(self, table: Optional[torch.Tensor] = None):
        """One batch, then the state advances.  Every refusal comes before the first launch."""
        st = self.store
        st._require_device()
        if table is not None:      # injected: its rows are read on the host and checked (a drawn table is never read)
            st.require_table(table, self.batchsize)
            check_rows(table.cpu().numpy(), st.n_frames, st.video_length)
        else:
            table = self.draw()
        color, geo = st.gather(table)
        self.last_table = table
        self.advance()
        return {"color": color, st.geometric_info: geo}

    def advance(self):
        """Move the state past one batch without making it (next_batch() does this after its launches)."""
        self.iteration += 1
        if self.iteration >= len(self):
            self.epoch, self.iteration = self.epoch + 1, 0

    def __iter__(self):
        while True:
            yield self.next_batch()
            if self.iteration == 0:
                return

    @property
    def launches_per_batch(self) -> int:
        """One draw, one gather per stream, one more launch for SURREAL depth."""
        return 1 + self.store.launches_per_gather

    def state_dict(self):
        return dict(seed=self.seed, epoch=self.epoch, iteration=self.iteration)

    def load_state_dict(self, sd):
        epoch, iteration = int(sd["epoch"]), int(sd["iteration"])
        if epoch < 0 or not 0 <= iteration < len(self):
            raise ValueError(f"ClipSampler: epoch {epoch}, iteration {iteration} of {len(self)}")
        self._fixed_seed, self.epoch, self.iteration = int(sd["seed"]), epoch, iteration
