"""RunMonitor: the training log kept on the device, and the sample log without a host round trip.

    mon = trainer.build_monitor(cfg, models, opts, interval=100, lecam=lc)
    runner = trainer.StepRunner(cfg, models, opts, loss, lecam=lc, monitor=mon)
    ...
    runner.step(xc, xg, t)               # one more launch per iteration; every `interval` iterations one more and an async copy of 8-byte words
    for rec in mon.poll():               # never blocks: the records whose copy has arrived, oldest first
        rec["slots"]["loss_gen"]["mean"], rec["groups"]["idis_real"]["frac_pos"], rec["first_iteration"], rec["last_iteration"]

The reference's trainer reads its four losses on the host every iteration (trainer.py:326-328,363: ``logger.update("loss_*", loss.cpu().item())``), averages them
between ``logger.log()`` calls (logger.py:144-148,280-283) and histograms / tiles its samples in numpy (trainer.py:109-169).  Here ``observe`` folds an iteration's
0-d device scalars and the discriminators' logits into a WINDOW — one tensor of 8-byte words in device memory — with one launch and no host read; ``roll``
publishes the window into a ring of device records, resets it, and starts the copy of that record into pinned host memory on a side stream.  The words:

    header   first iteration, last iteration, observations, rolls
    slot     sum f64, count, nonfinite, min f64, max f64, last f64            (per scalar: a loss, a gradient norm, a LeCam term)
    group    n, sum f64, sumsq f64, pos, neg, nonfinite                       (per logits tensor: D(real), D(fake) of each discriminator and phase)

``monitor_host`` is the numpy mirror of both kernels, word for word; ``hist_host`` and ``grid_host`` mirror the sample log's two kernels.

Data parallel: each rank monitors its own batch; no collective is added.
"""
from __future__ import annotations

import collections
import ctypes as C
import math
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from .native import NativeError, c_array, check, dims5, lib, ptr, stream_ptr

MAX_SLOTS, MAX_GROUPS, MAX_N = 32, 16, 1 << 24                                       # include/dcvgan_hip.h: DCV_MONITOR_*
HEADER_WORDS, SLOT_WORDS, GROUP_WORDS = 4, 6, 6
FIRST_ITERATION, LAST_ITERATION, OBSERVATIONS, ROLLS = range(4)
SLOT_SUM, SLOT_COUNT, SLOT_NONFINITE, SLOT_MIN, SLOT_MAX, SLOT_LAST = range(6)
GROUP_N, GROUP_SUM, GROUP_SUMSQ, GROUP_POS, GROUP_NEG, GROUP_NONFINITE = range(6)
F32, F64, I64 = np.float32, np.float64, np.int64


def state_words(n_slots: int, n_groups: int) -> int:
    return HEADER_WORDS + SLOT_WORDS * n_slots + GROUP_WORDS * n_groups


def _bits(v) -> int:
    """The bits of a double as the int64 the state holds."""
    return int(np.array([v], dtype=F64).view(I64)[0])


def fresh_state(n_slots: int, n_groups: int, first_iteration: int = 1) -> np.ndarray:
    """A window nothing has been observed in: zeros, every slot's min = +inf and max = -inf."""
    w = np.zeros(state_words(n_slots, n_groups), dtype=I64)
    w[FIRST_ITERATION] = first_iteration
    for s in range(n_slots):
        w[HEADER_WORDS + s * SLOT_WORDS + SLOT_MIN] = _bits(np.inf)
        w[HEADER_WORDS + s * SLOT_WORDS + SLOT_MAX] = _bits(-np.inf)
    return w


# ---- the numpy mirrors --------------------------------------------------------------------------------------------------------------------------------------------
def _lane_tree_sum(v: np.ndarray) -> float:
    """dcv_lecam_sums' order on doubles: lane l adds elements l, l + 256, ... into a double that starts at +0.0; then p[l] += p[l + s] for s = 128 .. 1."""
    v = np.asarray(v, dtype=F64).reshape(-1)
    rows = (v.size + 255) // 256
    pad = np.zeros(rows * 256, dtype=F64)      # (x + 0.0 == x for every x a running sum that started at +0.0 can hold: the padding adds nothing)
    pad[:v.size] = v
    p = np.zeros(256, dtype=F64)
    for r in pad.reshape(rows, 256):
        p = p + r
    s = 128
    while s >= 1:
        p[:s] = p[:s] + p[s:2 * s]
        s //= 2
    return float(p[0])


def monitor_host(state: np.ndarray, n_slots: int, n_groups: int, scalars: Optional[Sequence] = None, logits: Optional[Sequence] = None,
                 roll: Optional[int] = None):
    """The numpy mirror of dcv_monitor_observe and dcv_monitor_roll on an int64 word array (modified in place).

    ``scalars``: n_slots values (None = a null slot), ``logits``: n_groups arrays (None = a null group): one observe when either is given.
    ``roll=iteration``: afterwards one roll; -> the published record (a new array), else None."""
    w = state
    assert w.dtype == I64 and w.size == state_words(n_slots, n_groups)
    f = w.view(F64)
    if scalars is not None or logits is not None:
        scalars = [None] * n_slots if scalars is None else list(scalars)
        logits = [None] * n_groups if logits is None else list(logits)
        assert len(scalars) == n_slots and len(logits) == n_groups
        w[OBSERVATIONS] += 1
        with np.errstate(all="ignore"):
            for s, v in enumerate(scalars):
                if v is None:
                    continue
                o = HEADER_WORDS + s * SLOT_WORDS
                d = F64(F32(v))
                f[o + SLOT_LAST] = d
                if np.isfinite(d):
                    f[o + SLOT_SUM] = f[o + SLOT_SUM] + d
                    w[o + SLOT_COUNT] += 1
                    if d < f[o + SLOT_MIN]:
                        f[o + SLOT_MIN] = d
                    if d > f[o + SLOT_MAX]:
                        f[o + SLOT_MAX] = d
                else:
                    w[o + SLOT_NONFINITE] += 1
            for g, y in enumerate(logits):
                if y is None:
                    continue
                y = np.asarray(y, dtype=F32).reshape(-1)
                assert 1 <= y.size <= MAX_N
                o = HEADER_WORDS + n_slots * SLOT_WORDS + g * GROUP_WORDS
                ok = np.isfinite(y)
                d = np.where(ok, y, F32(0)).astype(F64)      # a skipped element and an added +0.0 leave the same bits
                w[o + GROUP_N] += y.size
                f[o + GROUP_SUM] = f[o + GROUP_SUM] + _lane_tree_sum(d)
                f[o + GROUP_SUMSQ] = f[o + GROUP_SUMSQ] + _lane_tree_sum(d * d)
                w[o + GROUP_POS] += int(np.count_nonzero(ok & (y > 0)))
                w[o + GROUP_NEG] += int(np.count_nonzero(ok & (y < 0)))
                w[o + GROUP_NONFINITE] += int(np.count_nonzero(~ok))
    if roll is None:
        return None
    record = w.copy()
    record[LAST_ITERATION] = roll
    rolls = int(w[ROLLS])
    w[:] = fresh_state(n_slots, n_groups, int(roll) + 1)
    w[LAST_ITERATION], w[ROLLS] = roll, rolls + 1
    return record


def hist_host(x: np.ndarray, channel: int = 0) -> np.ndarray:
    """dcv_hist_u8: the 256 counts of one channel of a uint8 (N, C, T, H, W) array, int64."""
    x = np.asarray(x)
    assert x.dtype == np.uint8 and x.ndim == 5 and 0 <= channel < x.shape[1]
    out = np.zeros(256, dtype=I64)
    for clip in x[:, channel]:                  # per clip run, as the kernel walks them
        vals, counts = np.unique(clip.reshape(-1), return_counts=True)
        out[vals] += counts
    return out


def grid_host(geo: np.ndarray, colour: np.ndarray, rows: int, cols: int) -> np.ndarray:
    """dcv_video_grid_u8 as the index arithmetic of its kernel: two uint8 (rows*cols, 3, T, H, W) arrays -> (1, T, 3, rows*H, 2*cols*W)."""
    geo, colour = np.asarray(geo), np.asarray(colour)
    n, ch, t, h, w = geo.shape
    assert geo.dtype == colour.dtype == np.uint8 and colour.shape == geo.shape and ch == 3 and n == rows * cols
    out = np.empty((1, t, 3, rows * h, 2 * cols * w), dtype=np.uint8)
    for side, src in enumerate((geo, colour)):
        for r in range(rows):
            for c in range(cols):
                x0 = (side * cols + c) * w
                out[0, :, :, r * h:(r + 1) * h, x0:x0 + w] = src[r * cols + c].transpose(1, 0, 2, 3)
    return out


def parse_record(words: np.ndarray, slots: Sequence[str], groups: Sequence[str]) -> dict:
    """A published record's words as a dict: per slot mean (sum / count in fp64, computed here; nan for an empty slot), count, nonfinite, min, max, last; per group
    n, mean and std over the finite logits (population std: sqrt(max(sumsq / m - mean^2, 0))), pos, neg, nonfinite, frac_pos = pos / m; the iteration range."""
    w = np.asarray(words, dtype=I64)
    f = w.view(F64)
    rec = dict(first_iteration=int(w[FIRST_ITERATION]), last_iteration=int(w[LAST_ITERATION]), observations=int(w[OBSERVATIONS]), rolls=int(w[ROLLS]),
               slots={}, groups={}, words=w)
    for s, name in enumerate(slots):
        o = HEADER_WORDS + s * SLOT_WORDS
        count = int(w[o + SLOT_COUNT])
        rec["slots"][name] = dict(mean=float(f[o + SLOT_SUM]) / count if count else math.nan, count=count, nonfinite=int(w[o + SLOT_NONFINITE]),
                                  min=float(f[o + SLOT_MIN]), max=float(f[o + SLOT_MAX]), last=float(f[o + SLOT_LAST]))
    for g, name in enumerate(groups):
        o = HEADER_WORDS + len(slots) * SLOT_WORDS + g * GROUP_WORDS
        n, bad, pos = int(w[o + GROUP_N]), int(w[o + GROUP_NONFINITE]), int(w[o + GROUP_POS])
        m = n - bad
        mean = float(f[o + GROUP_SUM]) / m if m else math.nan
        std = math.sqrt(max(float(f[o + GROUP_SUMSQ]) / m - mean * mean, 0.0)) if m else math.nan
        rec["groups"][name] = dict(n=n, mean=mean, std=std, pos=pos, neg=int(w[o + GROUP_NEG]), nonfinite=bad, frac_pos=pos / m if m else math.nan)
    return rec


# ---- the device side ----------------------------------------------------------------------------------------------------------------------------------------------
def _require_cuda(t, what: str, dtype):
    if not isinstance(t, torch.Tensor):
        raise NativeError(f"{what}: expected a device tensor, got {type(t).__name__}" +
                          (" — with sync_losses=True the iteration's values are Python floats, which the monitor does not upload" if isinstance(t, float) else ""))
    if not t.is_cuda:
        raise NativeError(f"{what}: expected a HIP device tensor, got {t.device} — the monitor runs on the GPU only (there is no CPU fallback)")
    if t.dtype != dtype:
        raise NativeError(f"{what}: expected {dtype}, got {t.dtype}")
    if t.device.index != torch.cuda.current_device():
        raise NativeError(f"{what}: tensor is on {t.device} but the current device is cuda:{torch.cuda.current_device()}")
    if not t.is_contiguous():
        raise NativeError(f"{what}: expected a contiguous tensor (the monitor never copies one)")


class RunMonitor:
    """``RunMonitor(slots, groups, device, ring=4)``: `slots` names up to 32 scalars of ``StepRunner.step()``'s result, `groups` up to 16 logits tensors.

    ``observe(out, logits)``: one launch, no host read, no torch kernel.  ``roll(iteration)``: one launch and one async copy; THE ONE WAIT of this class is here:
    when all `ring` records are still on their way to the host, the host waits for the oldest — which bounds its lead over the GPU to `ring` rolls, the way
    StepRunner.max_ahead bounds it in iterations.  ``poll()`` never blocks; ``drain()`` waits for every outstanding record.
    ``state``: the live window, an int64 device tensor (what RunState carries).  `interval` is StepRunner's: it rolls every `interval` iterations."""

    def __init__(self, slots: Sequence[str], groups: Sequence[str], device=None, ring: int = 4, interval: int = 100, first_iteration: int = 1):
        self.slots, self.groups = tuple(str(s) for s in slots), tuple(str(g) for g in groups)
        if len(self.slots) > MAX_SLOTS or len(self.groups) > MAX_GROUPS:
            raise ValueError(f"RunMonitor: at most {MAX_SLOTS} slots and {MAX_GROUPS} groups, got {len(self.slots)} and {len(self.groups)}")
        if len(set(self.slots)) != len(self.slots) or len(set(self.groups)) != len(self.groups):
            raise ValueError("RunMonitor: slot and group names are distinct")
        if int(ring) < 1 or int(interval) < 1:
            raise ValueError(f"RunMonitor: ring >= 1 and interval >= 1, got {ring!r}, {interval!r}")
        from . import util
        self.device = torch.device(device if device is not None else util.current_device())
        self.ring, self.interval = int(ring), int(interval)
        self.words = state_words(len(self.slots), len(self.groups))
        # host tensors copied to the device once (no kernel)
        self.state = torch.from_numpy(fresh_state(len(self.slots), len(self.groups), first_iteration)).to(self.device)
        self._records: List[Optional[torch.Tensor]] = [None] * self.ring      # device records and their pinned host twins, made by the first roll
        self._hosts: List[Optional[torch.Tensor]] = [None] * self.ring
        self._done: List[Optional["torch.cuda.Event"]] = [None] * self.ring
        self._flight = collections.deque()      # ring slots whose copy is under way, oldest first
        self._ready: List[dict] = []            # records harvested by roll()'s wait, not yet handed out
        self._side = None
        self.rolled = 0                         # rolls issued: the ring position is rolled % ring
        self.observed = 0

    # ---- observe --------------------------------------------------------------------------------------------------------------------------------------------
    def observe(self, out: Dict[str, torch.Tensor], logits: Optional[Dict[str, Optional[torch.Tensor]]] = None, from_lanes: bool = False):
        """`out`: name -> 0-d fp32 device tensor (a missing name or None: the slot is not observed this iteration); `logits`: group name -> contiguous fp32 device
        tensor of 1 .. 2^24 elements, or None.  Every refusal (NativeError) comes before the launch; nothing is copied, nothing but the window is written.
        `from_lanes=True`: the logits were allocated on other streams (which the caller has made the current one wait for) and are given `record_stream` here;
        StepRunner's are recorded on the main stream when its lanes join, so it leaves this off."""
        if self.state.device.type != "cuda":
            raise NativeError(f"RunMonitor: the state is on {self.state.device} — the monitor runs on the GPU only (there is no CPU fallback)")
        logits = logits or {}
        unknown = [k for k in logits if k not in self.groups]
        if unknown:
            raise NativeError(f"RunMonitor.observe: unknown logit groups {unknown} (built for {list(self.groups)})")
        held, lanes = [], []      # the tensors stay referenced until the launch is enqueued
        cur = torch.cuda.current_stream(self.device) if from_lanes else None
        sp, gp, gn = [], [], []
        for name in self.slots:
            t = out.get(name)
            if t is None:
                sp.append(0)
                continue
            _require_cuda(t, f"RunMonitor.observe: {name}", torch.float32)
            if t.numel() != 1:
                raise NativeError(f"RunMonitor.observe: {name}: expected one value, got {tuple(t.shape)}")
            held.append(t)
            sp.append(t.data_ptr())
        for name in self.groups:
            t = logits.get(name)
            if t is None:
                gp.append(0); gn.append(0)
                continue
            _require_cuda(t, f"RunMonitor.observe: {name}", torch.float32)
            if not 1 <= t.numel() <= MAX_N:
                raise NativeError(f"RunMonitor.observe: {name}: 1 to 2^24 logits, got {t.numel()}")
            held.append(t)
            if from_lanes:
                lanes.append(t)
            gp.append(t.data_ptr()); gn.append(t.numel())
        for t in lanes:
            t.record_stream(cur)      # allocated on a lane, read here on the caller's stream
        check(lib().dcv_monitor_observe(len(sp), c_array(sp), len(gp), c_array(gp), c_array(gn, C.c_int64), ptr(self.state), stream_ptr()), "dcv_monitor_observe")
        self.observed += 1
        del held

    # ---- roll, poll, drain ------------------------------------------------------------------------------------------------------------------------------------
    def _harvest(self, k: int) -> dict:
        rec = parse_record(self._hosts[k].numpy().copy(), self.slots, self.groups)
        self._done[k] = None
        return rec

    def roll(self, iteration: int):
        """Publish the window as the record of iterations first .. `iteration`, reset it, and start the record's copy to the host on a side stream."""
        if self.state.device.type != "cuda":
            raise NativeError(f"RunMonitor: the state is on {self.state.device} — the monitor runs on the GPU only (there is no CPU fallback)")
        k = self.rolled % self.ring
        if self._records[k] is None:
            self._records[k] = torch.empty(self.words, dtype=torch.int64, device=self.device)
            self._hosts[k] = torch.empty(self.words, dtype=torch.int64, pin_memory=True)
        while k in self._flight:      # all `ring` records are in flight: wait for the oldest (the only wait of this class)
            j = self._flight.popleft()
            self._done[j].synchronize()
            self._ready.append(self._harvest(j))
        cur = torch.cuda.current_stream(self.device)
        if self._side is None:
            self._side = torch.cuda.Stream(self.device)
        check(lib().dcv_monitor_roll(len(self.slots), len(self.groups), ptr(self.state), ptr(self._records[k]), int(iteration), stream_ptr()), "dcv_monitor_roll")
        published = torch.cuda.Event()
        published.record(cur)
        self._side.wait_event(published)
        with torch.cuda.stream(self._side):
            self._hosts[k].copy_(self._records[k], non_blocking=True)
            done = torch.cuda.Event()
            done.record(self._side)
        self._done[k] = done
        self._flight.append(k)
        self.rolled += 1

    def poll(self) -> List[dict]:
        """The records whose copy has completed, oldest first.  Never blocks."""
        while self._flight and self._done[self._flight[0]].query():
            self._ready.append(self._harvest(self._flight.popleft()))
        out, self._ready = self._ready, []
        return out

    def drain(self) -> List[dict]:
        """Every outstanding record, oldest first; the host waits for their copies."""
        while self._flight:
            k = self._flight.popleft()
            self._done[k].synchronize()
            self._ready.append(self._harvest(k))
        out, self._ready = self._ready, []
        return out

    # ---- host reads: checkpoints only -------------------------------------------------------------------------------------------------------------------------
    def state_dict(self):
        return dict(state=[int(v) for v in self.state.cpu().tolist()], slots=list(self.slots), groups=list(self.groups), interval=self.interval, rolled=self.rolled)

    def load_state_dict(self, sd):
        if list(sd["slots"]) != list(self.slots) or list(sd["groups"]) != list(self.groups):
            raise ValueError(f"RunMonitor: built for slots {list(self.slots)} and groups {list(self.groups)}, the checkpoint holds {list(sd['slots'])} and {list(sd['groups'])}")
        words = [int(v) for v in sd["state"]]
        if len(words) != self.words:
            raise ValueError(f"RunMonitor: the state has {self.words} words, the checkpoint {len(words)}")
        self.state.copy_(torch.tensor(words, dtype=torch.int64))
        self.interval, self.rolled = int(sd["interval"]), int(sd["rolled"])


# ---- the sample log -----------------------------------------------------------------------------------------------------------------------------------------------
def _require_u8(t, what: str):
    _require_cuda(t, what, torch.uint8)
    if t.dim() != 5:
        raise NativeError(f"{what}: expected (N, C, T, H, W), got {tuple(t.shape)}")


def hist_u8(x: torch.Tensor, channel: int = 0, counts: Optional[torch.Tensor] = None, accumulate: bool = False) -> torch.Tensor:
    """The 256 int64 counts of one channel of a contiguous uint8 device tensor (N, C, T, H, W) (dcv_hist_u8); `counts`: an existing table, added to with
    `accumulate`.  Stays on the device."""
    _require_u8(x, "hist_u8 input")
    if counts is None:
        if accumulate:
            raise NativeError("hist_u8: accumulate needs the counts to add to")
        counts = torch.empty(256, dtype=torch.int64, device=x.device)
    else:
        _require_cuda(counts, "hist_u8 counts", torch.int64)
        if counts.numel() != 256:
            raise NativeError(f"hist_u8 counts: expected 256 values, got {tuple(counts.shape)}")
    n, c, t, h, w = x.shape
    check(lib().dcv_hist_u8(ptr(x), n, c, t, h, w, int(channel), ptr(counts), int(bool(accumulate)), stream_ptr()), "dcv_hist_u8")
    return counts


def video_grid_u8(geo: torch.Tensor, colour: torch.Tensor, rows: int, cols: int) -> torch.Tensor:
    """Two contiguous uint8 device tensors (rows*cols, 3, T, H, W) -> the (1, T, 3, rows*H, 2*cols*W) mosaic (dcv_video_grid_u8).  Stays on the device."""
    _require_u8(geo, "video_grid_u8 geometry")
    _require_u8(colour, "video_grid_u8 colour")
    if geo.shape != colour.shape or geo.shape[1] != 3:
        raise NativeError(f"video_grid_u8: expected two (N, 3, T, H, W) tensors, got {tuple(geo.shape)} and {tuple(colour.shape)}")
    n, _, t, h, w = geo.shape
    out = torch.empty((1, t, 3, rows * h, 2 * cols * w), dtype=torch.uint8, device=geo.device)
    check(lib().dcv_video_grid_u8(ptr(geo), ptr(colour), int(rows), int(cols), n, t, h, w, ptr(out), stream_ptr()), "dcv_video_grid_u8")
    return out


def _geometry_u8_into(xg: torch.Tensor, geometric_info: str, out: torch.Tensor):
    """sampling.geometry_to_color's conversions, written into the contiguous uint8 (B, 3, T, H, W) device slice `out`."""
    from . import sampling
    L, s = lib(), stream_ptr()
    xd = dims5(xg)
    if geometric_info == "depth":
        check(L.dcv_videos_to_uint8(ptr(xg), C.byref(xd), ptr(out), 3, s), "dcv_videos_to_uint8")
    elif geometric_info == "optical-flow":
        b, _, t, h, _ = xg.shape
        mm = torch.empty(2 * b * t, dtype=torch.float32, device=xg.device)
        check(L.dcv_flow_to_rgb(ptr(xg), C.byref(xd), float(h), ptr(out), ptr(mm), s), "dcv_flow_to_rgb")
    elif geometric_info == "segmentation":
        if xg.shape[1] != len(sampling.SEGM_PALETTE_U8):
            raise NativeError(f"segmentation visualisation expects {len(sampling.SEGM_PALETTE_U8)} part channels, got {xg.shape[1]}")
        pal = torch.tensor(sampling.SEGM_PALETTE_U8, dtype=torch.uint8).to(xg.device)
        check(L.dcv_segm_to_rgb(ptr(xg), C.byref(xd), ptr(pal), ptr(out), s), "dcv_segm_to_rgb")
    else:
        raise NotImplementedError(f"geometry visualisation for {geometric_info!r}")


def sample_log(ggen, cgen, num: int, rows: int, cols: int, batchsize: Optional[int] = None, real=None) -> dict:
    """Trainer.log_samples (trainer.py:109-169) on the device: `num = rows * cols` samples generated as sampling.generate_samples does (eval mode, no_grad, batches
    of `batchsize`, default `num` as the reference calls it), converted to uint8 on the device, channel 0 of both histogrammed, the two mosaics joined; only the
    grid and the two 256-bin count vectors are copied to the host.  ``real=(xg, xc)``: a real batch of float device clips takes the generated samples' place
    (trainer.py:146-169; its first `num` clips).
    -> {"video": uint8 (1, T, 3, rows*H, 2*cols*W), "hist_geo": int64[256], "hist_colour": int64[256]}: what tf_log_video and a histogram writer take."""
    from .native import _require
    num, rows, cols = int(num), int(rows), int(cols)
    if num < 1 or rows * cols != num:
        raise NativeError(f"sample_log: {num} samples do not fill a {rows} x {cols} grid")
    batchsize = num if batchsize is None else int(batchsize)
    if batchsize < 1:
        raise NativeError(f"sample_log: batchsize >= 1, got {batchsize}")
    geo = col = None

    def convert(xg, xc, a):
        nonlocal geo, col
        _require(xg, "sample_log geometry clips")
        _require(xc, "sample_log colour clips")
        if xg.dim() != 5 or xc.dim() != 5 or xc.shape[1] != 3:
            raise NativeError(f"sample_log: expected (B, C, T, H, W) clips with 3 colour channels, got {tuple(xg.shape)} and {tuple(xc.shape)}")
        k = min(xg.shape[0], num - a)
        if geo is None:
            shape = (num, 3) + tuple(xc.shape[2:])
            geo, col = torch.empty(shape, dtype=torch.uint8, device=xc.device), torch.empty(shape, dtype=torch.uint8, device=xc.device)
        xg, xc = xg[:k], xc[:k]      # views of the first k clips: the last batch is truncated
        if tuple(xc.shape[2:]) != tuple(geo.shape[2:]) or tuple(xg.shape[2:]) != tuple(geo.shape[2:]):
            raise NativeError(f"sample_log: clips of {tuple(xg.shape[2:])} and {tuple(xc.shape[2:])} in a log of {tuple(geo.shape[2:])}")
        _geometry_u8_into(xg, ggen.geometric_info, geo[a:a + k])
        xd = dims5(xc)
        check(lib().dcv_videos_to_uint8(ptr(xc), C.byref(xd), ptr(col[a:a + k]), 1, stream_ptr()), "dcv_videos_to_uint8")
        return k

    if real is not None:
        xg, xc = real
        if xg.shape[0] < num or xc.shape[0] < num:
            raise NativeError(f"sample_log: the real batch holds {xg.shape[0]} clips, the grid needs {num}")
        convert(xg.detach(), xc.detach(), 0)
    else:
        ggen.eval()
        cgen.eval()
        for a in range(0, num, batchsize):
            with torch.no_grad():
                xg = ggen.sample_videos(batchsize)
                xc = cgen.forward_videos(xg)
            convert(xg, xc, a)
    hg, hc = hist_u8(geo, 0), hist_u8(col, 0)
    video = video_grid_u8(geo, col, rows, cols)
    return {"video": video.cpu().numpy(), "hist_geo": hg.cpu().numpy(), "hist_colour": hc.cpu().numpy()}
