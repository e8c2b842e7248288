"""RunState: everything a training run has become — snapshot, fingerprint, rollback and exact resume, on the device.

    rs = trainer.build_run_state(cfg, models, opts, runner=runner, ema=ema, spectral=sn, augment=aug, lecam=lc, sampler=sampler, extra=mine)
    snap = rs.capture()                  # after runner.step(...): the state as that iteration leaves it, packed into a device arena on the current stream
    snap.restore()                       # rollback: the live tensors and every host scalar are as they were at the capture
    snap.save(path); rs2.load(path).restore()      # resume in fresh objects, bit for bit
    rs.fingerprint()                     # (n_entries, 2) int64 on the device: a 128-bit digest per state tensor, without a copy
    RunState.diff(a.fingerprint_host(), b.fingerprint_host())      # the names of the entries that differ

The state is a MANIFEST — an ordered list of named device tensors, handled as 32-bit words — and a dict of host scalars beside it.  ``capture()`` is
dcv_state_pack_multi over the manifest into a preallocated arena (a ring of ``slots`` arenas): no host read, no torch kernel, no allocation after the first call.
The host scalars (step counts, hyper-parameters, random streams' counters, the iteration number, the sampler's position, ``extra``) are copied at call time: they
describe exactly the iteration just enqueued, which is the stream position the pack sees.

The digest of a tensor of dwords w[0 .. n): h_i = splitmix64-finaliser(i * 0x9E3779B97F4A7C15 + w[i]) mod 2^64, the pair (sum of h_i mod 2^64, xor of h_i): exact
and independent of the order of traversal.  ``digest_host`` is the numpy mirror of the kernels.

Random streams: a ``PhiloxRng`` without a fixed seed follows ``torch.initial_seed()`` and starts over at counter 0 when that changes.  ``restore()`` therefore gives
such a stream ``fixed_seed = seed_seen`` when torch's current initial seed differs from the saved ``seed_seen`` (a resume in a process seeded otherwise); torch's
global seed is not touched.  ``t_rand`` is the caller's argument to ``StepRunner.step``: the generator behind it is the caller's state and belongs into ``extra``.

16-bit data paths: their channels-last twins and packed weights are caches keyed on the tensors' version counters, which ``restore()`` bumps; they are not state.

Host tensors (models built on the CPU: checkpoint tooling, tests without a GPU) are packed, unpacked and digested by the numpy mirror; nothing here trains there.
"""
from __future__ import annotations

import copy
import ctypes as C
from collections import OrderedDict
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from .native import NativeError, c_array, check, lib, ptr, stream_ptr

FORMAT_VERSION = 1
MT = 24                # tensors per launch (the multi-tensor table of DESIGN §10a)
MAX_DWORDS = 1 << 32
_GOLD, _MUL1, _MUL2 = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB
_DTYPES = {str(d): d for d in (torch.float32, torch.int32, torch.int64, torch.float64, torch.uint8)}
AUGMENT_RULE = ("adaptive", "target", "interval", "p_max", "adjust_clips", "batch", "mask", "max_dx", "max_dy", "cut_size", "contrast", "brightness")
LECAM_RULE = ("n_dis", "weight", "decay", "start", "one_sided")


def _words(array) -> np.ndarray:
    """The array's bytes as a flat uint32 view (a copy only where the input is not contiguous)."""
    if isinstance(array, torch.Tensor):
        if array.element_size() % 4:
            raise NativeError(f"runstate: state is handled as 32-bit words, got {array.dtype}")
        array = array.detach().cpu().contiguous().numpy()
    a = np.ascontiguousarray(array)
    if a.dtype.itemsize % 4:
        raise NativeError(f"runstate: state is handled as 32-bit words, got {a.dtype}")
    return a.reshape(-1).view(np.uint32)


def digest_host(array) -> Tuple[int, int]:
    """(sum, xor) of the array's dwords as unsigned Python integers: what the kernels leave in a row of the digest table."""
    w = _words(array)
    if w.size >= MAX_DWORDS:
        raise NativeError(f"runstate: a tensor of {w.size} dwords: 0 <= dwords < 2^32")
    s, x = np.uint64(0), np.uint64(0)
    with np.errstate(over="ignore"):
        for a in range(0, w.size, 1 << 22):
            part = w[a:a + (1 << 22)].astype(np.uint64)
            z = np.arange(a, a + part.size, dtype=np.uint64) * np.uint64(_GOLD) + part
            z ^= z >> np.uint64(30)
            z *= np.uint64(_MUL1)
            z ^= z >> np.uint64(27)
            z *= np.uint64(_MUL2)
            z ^= z >> np.uint64(31)
            s = s + np.add.reduce(z, dtype=np.uint64)
            x = x ^ np.bitwise_xor.reduce(z)
    return int(s), int(x)


def _signed(pair) -> List[int]:
    """An unsigned digest pair as the two int64 values the device table holds."""
    return [int(v) for v in np.array(pair, dtype=np.uint64).view(np.int64)]


def _padded(dwords: int) -> int:
    return (dwords + 3) // 4 * 4


def _entry_key(e) -> tuple:
    return (e["name"], e["dtype"], tuple(e["shape"]))


class _Layout:
    """The manifest of one set of live tensors and the argument arrays of the C calls, valid while ``key`` — names and data_ptr()s — stays the same."""

    def __init__(self, key, items):
        self.key = key
        self.names = [n for n, _ in items]
        self.tensors = [t for _, t in items]
        devs = {t.device for t in self.tensors}
        if len(devs) > 1:
            raise NativeError(f"RunState: the state lives on several devices ({sorted(str(d) for d in devs)})")
        self.device = devs.pop() if devs else torch.device("cpu")
        self.manifest, off = [], 0
        for n, t in items:
            if t.element_size() % 4:
                raise NativeError(f"RunState: {n}: state is handled as 32-bit words, got {t.dtype}")
            if str(t.dtype) not in _DTYPES:
                raise NativeError(f"RunState: {n}: unsupported dtype {t.dtype}")
            if not t.is_contiguous():
                raise NativeError(f"RunState: {n}: state tensors must be contiguous")
            dwords = t.numel() * (t.element_size() // 4)
            if dwords >= MAX_DWORDS:
                raise NativeError(f"RunState: {n}: {dwords} dwords: 0 <= dwords < 2^32 per tensor")
            if self.device.type == "cuda" and t.device.index != torch.cuda.current_device():
                raise NativeError(f"RunState: {n} is on {t.device} but the current device is cuda:{torch.cuda.current_device()}")
            self.manifest.append(dict(name=n, dtype=str(t.dtype), shape=tuple(int(v) for v in t.shape), dwords=dwords, offset=off))
            off += _padded(dwords)
        self.total = off      # dwords
        self.n = len(items)
        self.src = c_array(self.tensors)
        self.dwords = c_array([e["dwords"] for e in self.manifest], C.c_int64)
        self.offsets = c_array([e["offset"] for e in self.manifest], C.c_int64)
        self.launches = sum((1 if any(e["dwords"] for e in self.manifest[a:a + MT]) else 0) + 1 for a in range(0, self.n, MT))


def _segments(manifest, arena_bytes: int):
    """Checks a stored manifest against its arena's size; -> the total in dwords."""
    off = 0
    for e in manifest:
        if int(e["offset"]) != off or int(e["offset"]) % 4:
            raise NativeError(f"runstate: entry {e['name']} starts at dword {e['offset']}, expected {off}")
        off += _padded(int(e["dwords"]))
    if off * 4 != arena_bytes and not (off == 0 and arena_bytes == 16):
        raise NativeError(f"runstate: the manifest describes {off * 4} bytes, the arena holds {arena_bytes}")
    return off


class Snapshot:
    """One captured state: a manifest, the host scalars, an arena and its digests.  ``restore()`` applies it to the RunState's live objects; ``save()`` writes it."""

    def __init__(self, owner: "RunState", manifest, host, arena: torch.Tensor, digests: torch.Tensor, slot: Optional[int], gen: int = 0):
        self.owner, self.manifest, self.host, self.arena, self.digests, self.slot, self.gen = owner, manifest, host, arena, digests, slot, gen

    def _alive(self):
        if self.slot is not None and (self.owner._arenas[self.slot] is not self.arena or self.owner._gen[self.slot] != self.gen):
            raise NativeError(f"Snapshot: its arena (slot {self.slot} of a ring of {self.owner.slots}) has been overwritten by a later capture()")

    @torch.no_grad()
    def restore(self):
        """The live tensors and every host scalar become what they were at the capture.  Every refusal comes before anything is written."""
        self._alive()
        rs = self.owner
        rs._check(self.manifest, self.host)
        rs._shape_optimizers(self.manifest, self.host)
        lay = rs._layout()
        if [_entry_key(e) for e in lay.manifest] != [_entry_key(e) for e in self.manifest]:
            raise NativeError("Snapshot.restore: the live state does not take the snapshot's layout (" + rs._first_difference(self.manifest, lay.manifest) + ")")
        if lay.device != self.arena.device:
            raise NativeError(f"Snapshot.restore: the arena is on {self.arena.device}, the live state on {lay.device}")
        if lay.device.type == "cuda":
            dst = c_array(lay.tensors)
            check(lib().dcv_state_unpack_multi(lay.n, dst, lay.dwords, ptr(self.arena), lay.total, lay.offsets, stream_ptr()), "dcv_state_unpack_multi")
        else:
            words = self.arena.numpy().view(np.uint32)
            for e, t in zip(lay.manifest, lay.tensors):
                if e["dwords"]:
                    _words_view(t)[:] = words[e["offset"]:e["offset"] + e["dwords"]]
        if lay.tensors:
            # the copy wrote through raw pointers: the packed-weight caches are keyed on the version counters, as in Adam.step and ModelEma.update
            torch.autograd.graph.increment_version(lay.tensors)
        rs._set_host(self.host)
        if rs.spectral is not None:
            if lay.device.type == "cuda":
                rs.spectral.refresh()      # sigma and W / sigma of the restored weights and u, v: bit for bit what the run held (its own formulas, no power iteration)
            else:
                for c in rs.spectral.convs:
                    c.__dict__["_dcv_spectral"].version = None

    def save(self, path):
        """ONE file (torch.save): format version, manifest, host scalars, digests and the arena as a uint8 tensor.  The device -> pinned host copy runs on a side
        stream behind an event of the current one; the host waits for that copy alone."""
        self._alive()
        arena, digests = self.arena, self.digests
        if arena.is_cuda:
            cur = torch.cuda.current_stream(arena.device)
            side = self.owner._side_stream(arena.device)
            reached = torch.cuda.Event()
            reached.record(cur)
            side.wait_event(reached)
            with torch.cuda.stream(side):
                h_arena = torch.empty(arena.shape, dtype=arena.dtype, pin_memory=True)
                h_digests = torch.empty(digests.shape, dtype=digests.dtype, pin_memory=True)
                h_arena.copy_(arena, non_blocking=True)
                h_digests.copy_(digests, non_blocking=True)
                done = torch.cuda.Event()
                done.record(side)
            arena.record_stream(side)
            digests.record_stream(side)
            done.synchronize()
        else:
            h_arena, h_digests = arena, digests
        torch.save(dict(format=FORMAT_VERSION, manifest=[dict(e, shape=tuple(e["shape"])) for e in self.manifest], host=self.host, digests=h_digests, arena=h_arena), path)


def _words_view(t: torch.Tensor) -> np.ndarray:
    """A writable flat uint32 view of a contiguous host tensor's memory."""
    return t.detach().numpy().reshape(-1).view(np.uint32)


class RunState:
    def __init__(self, models, optimizers, runner=None, ema=None, spectral=None, augment=None, lecam=None, sampler=None, rngs=(), extra=None, slots: int = 2,
                 monitor=None):
        if int(slots) < 1:
            raise ValueError(f"RunState: slots >= 1, got {slots!r}")
        if extra is not None and not isinstance(extra, dict):
            raise ValueError("RunState: extra is a dict of plain values")
        self.models, self.optimizers, self.runner, self.ema, self.spectral, self.augment, self.lecam, self.sampler = \
            models, optimizers, runner, ema, spectral, augment, lecam, sampler
        self.rngs, self.extra, self.slots = tuple(rngs), extra, int(slots)
        # monitor.RunMonitor: its live window is one more entry and its names, interval and ring position one more block of host scalars; records already published
        # (on their way to the host or waiting for poll()) are the caller's and are not part of the state.  None: manifests and files are what they are without it
        self.monitor = monitor
        self._lay: Optional[_Layout] = None
        self._arenas: List[Optional[torch.Tensor]] = [None] * self.slots
        self._digests: List[Optional[torch.Tensor]] = [None] * self.slots
        self._gen = [0] * self.slots
        self._next = 0
        self._ws: Optional[torch.Tensor] = None
        self._fp: Optional[torch.Tensor] = None
        self._side = None

    # ---- what the state is --------------------------------------------------------------------------------------------------------------------------------
    def _model_names(self):
        from .trainer import MODEL_NAMES
        return [n for n in MODEL_NAMES if n in self.models] + [n for n in self.models if n not in MODEL_NAMES]

    def _opts(self):
        from .trainer import MODEL_NAMES
        names = [n for n in MODEL_NAMES if n in self.optimizers] + [n for n in self.optimizers if n not in MODEL_NAMES]
        return [(n, getattr(self.optimizers[n], "inner", self.optimizers[n])) for n in names]      # (a DataParallelAdam's state is its inner optimiser's)

    def _guards(self):
        out = []
        for _, o in self._opts():
            g = getattr(o, "guard", None)
            if g is not None and all(g is not h for h in out):
                out.append(g)
        return out

    def _philox(self):
        """Every distinct PhiloxRng of the run, in a fixed order: the process-wide stream, the models' own, the twins', the augmentation's, the caller's."""
        from . import rng as R
        cand = [R.default_rng()] + [getattr(self.models[n], "_rng", None) for n in self._model_names()]
        cand += [getattr(self.ema, "rng", None), getattr(self.augment, "rng", None)] + list(self.rngs)
        out = []
        for r in cand:
            if isinstance(r, R.PhiloxRng) and all(r is not q for q in out):
                out.append(r)
        return out

    @staticmethod
    def _blocks_of(name, o):
        """Per parameter of a guarded optimiser the manifest name of its step block (None without state): distinct blocks numbered in parameter order."""
        seen, out = {}, []
        for p in o.params:
            s = o.state.get(p)
            if s is None or "step_block" not in s:
                out.append(None)
                continue
            j = seen.setdefault(s["step_block"].data_ptr(), len(seen))
            out.append(f"optim.{name}.step_block.{j}")
        return out

    def _entries(self):
        out = []
        for n in self._model_names():
            out += [(f"model.{n}.{k}", t) for k, t in self.models[n].state_dict(keep_vars=True).items()]
        opts = self._opts()
        for n, o in opts:
            for i, p in enumerate(o.params):
                s = o.state.get(p)
                if s is not None:
                    out += [(f"optim.{n}.{i}.exp_avg", s["exp_avg"]), (f"optim.{n}.{i}.exp_avg_sq", s["exp_avg_sq"])]
        for n, o in opts:
            if getattr(o, "guard", None) is None:
                continue
            done = set()
            for p, b in zip(o.params, self._blocks_of(n, o)):
                if b is not None and b not in done:
                    done.add(b)
                    out.append((b, o.state[p]["step_block"]))
        for k, g in enumerate(self._guards()):
            if g.state is not None:
                out.append((f"guard.{k}.state", g.state))
        if self.ema is not None:
            for n in self.ema.names:
                out += [(f"ema.{n}.{k}", t) for k, t in self.ema.twins[n].state_dict(keep_vars=True).items()]
            out += [(f"ema_count.{n}", self.ema._blocks[n]) for n in self.ema.names]
        if self.augment is not None:
            out.append(("augment.state", self.augment.state))
        if self.lecam is not None:
            out.append(("lecam.state", self.lecam.state))
        if self.monitor is not None:
            out.append(("monitor.state", self.monitor.state))
        return out

    def _layout(self) -> _Layout:
        items = self._entries()
        key = tuple((n, t.data_ptr(), t.dtype, tuple(t.shape)) for n, t in items)
        if self._lay is None or self._lay.key != key:
            self._lay = _Layout(key, items)
        return self._lay

    def manifest(self) -> List[dict]:
        """The ordered entries of the live state: name, dtype, shape, dwords and arena offset (in dwords, a multiple of 4: 16 bytes)."""
        return [dict(e) for e in self._layout().manifest]

    def arena_bytes(self) -> int:
        return self._layout().total * 4

    def launches_per_capture(self) -> int:
        """Per table of 24 entries one pack launch (none for a table without dwords) and one launch that folds the digests' partials."""
        return self._layout().launches

    def _host_scalars(self) -> dict:
        h = dict(optim={}, guards=[], rngs=[r.state_dict() for r in self._philox()])
        for n, o in self._opts():
            guarded = getattr(o, "guard", None) is not None
            steps = [None if (guarded or o.state.get(p) is None) else int(o.state[p]["step"]) for p in o.params]
            h["optim"][n] = dict(lr=o.lr, betas=tuple(o.betas), eps=o.eps, weight_decay=o.weight_decay, grad_scale=o.grad_scale, guarded=guarded, steps=steps,
                                 blocks=self._blocks_of(n, o) if guarded else [None] * len(o.params))
        for g in self._guards():
            d = {k: getattr(g, k) for k in g.RULE}
            d["measurements"] = g.measurements
            h["guards"].append(d)
        h["iteration"] = None if self.runner is None else int(self.runner.iteration)
        h["sampler"] = None if self.sampler is None else dict(self.sampler.state_dict())
        h["ema"] = None if self.ema is None else dict(decay=self.ema.decay, warmup=self.ema.warmup)
        h["augment"] = None if self.augment is None else {k: getattr(self.augment, k) for k in AUGMENT_RULE}
        h["lecam"] = None if self.lecam is None else {k: getattr(self.lecam, k) for k in LECAM_RULE}
        h["spectral"] = None if self.spectral is None else dict(eps=self.spectral.eps)
        h["extra"] = copy.deepcopy(self.extra)
        if self.monitor is not None:      # (no key at all without one: the host scalars of such a run are what they were)
            h["monitor"] = dict(slots=list(self.monitor.slots), groups=list(self.monitor.groups), interval=self.monitor.interval, rolled=self.monitor.rolled)
        return h

    # ---- compatibility of a snapshot with the live objects ----------------------------------------------------------------------------------------------
    @staticmethod
    def _first_difference(theirs, mine) -> str:
        for a, b in zip(theirs, mine):
            if _entry_key(a) != _entry_key(b):
                return f"entry {a['name']}: the snapshot holds {a['dtype']}{tuple(a['shape'])}, the live state {b['name']} {b['dtype']}{tuple(b['shape'])}"
        if len(theirs) > len(mine):
            return f"entry {theirs[len(mine)]['name']}: not part of the live state"
        if len(mine) > len(theirs):
            return f"entry {mine[len(theirs)]['name']}: not part of the snapshot"
        return "no difference"

    def _check(self, manifest, host):
        """Raises NativeError naming the first entry of `manifest` that the live objects cannot take.  Optimiser state is compared with the parameters (the live
        optimiser may hold none yet, or more than the snapshot); everything else with the live tensors, in order.  Writes nothing."""
        is_opt = lambda e: e["name"].startswith("optim.")
        theirs = [e for e in manifest if not is_opt(e)]
        mine = [e for e in self._layout().manifest if not is_opt(e)]
        if [_entry_key(e) for e in theirs] != [_entry_key(e) for e in mine]:
            raise NativeError("RunState: the snapshot does not fit the live objects: " + self._first_difference(theirs, mine))
        opts = dict(self._opts())
        if sorted(host["optim"]) != sorted(opts):
            raise NativeError(f"RunState: the snapshot holds optimisers {sorted(host['optim'])}, the live run {sorted(opts)}")
        for n, o in opts.items():
            info = host["optim"][n]
            if bool(info["guarded"]) != (getattr(o, "guard", None) is not None) or len(info["steps"]) != len(o.params):
                raise NativeError(f"RunState: optimiser {n}: the snapshot's is {'guarded' if info['guarded'] else 'unguarded'} over {len(info['steps'])} parameters, "
                                  f"the live one {'guarded' if getattr(o, 'guard', None) is not None else 'unguarded'} over {len(o.params)}")
        for e in manifest:
            if not is_opt(e):
                continue
            parts = e["name"].split(".")
            o = opts.get(parts[1])
            if o is None:
                raise NativeError(f"RunState: entry {e['name']}: no such optimiser in the live run")
            if parts[2] == "step_block":
                want = ("torch.int32", (16,))
            else:
                i = int(parts[2])
                if i >= len(o.params):
                    raise NativeError(f"RunState: entry {e['name']}: the live optimiser has {len(o.params)} parameters")
                want = (str(o.params[i].dtype), tuple(o.params[i].shape))
            if (e["dtype"], tuple(e["shape"])) != want:
                raise NativeError(f"RunState: entry {e['name']}: the snapshot holds {e['dtype']}{tuple(e['shape'])}, the live parameter asks for {want[0]}{want[1]}")
        for what, live in (("iteration", self.runner), ("sampler", self.sampler), ("ema", self.ema), ("augment", self.augment), ("lecam", self.lecam),
                           ("spectral", self.spectral)):
            if (host[what] is None) != (live is None):
                raise NativeError(f"RunState: {what}: " + ("the snapshot has none, the live run has one" if host[what] is None else "the snapshot has one, the live run none"))
        theirs_mon = host.get("monitor")
        if (theirs_mon is None) != (self.monitor is None):
            raise NativeError("RunState: monitor: " + ("the snapshot has none, the live run has one" if theirs_mon is None else "the snapshot has one, the live run none"))
        if theirs_mon is not None:
            for k, mine_k in (("slots", list(self.monitor.slots)), ("groups", list(self.monitor.groups))):
                if list(theirs_mon[k]) != mine_k:
                    raise NativeError(f"RunState: monitor: the snapshot's {k} are {list(theirs_mon[k])}, the live monitor's {mine_k}")
        if len(host["rngs"]) != len(self._philox()) or len(host["guards"]) != len(self._guards()):
            raise NativeError(f"RunState: the snapshot holds {len(host['rngs'])} random streams and {len(host['guards'])} guards, the live run "
                              f"{len(self._philox())} and {len(self._guards())}")
        if (host["extra"] is None) != (self.extra is None):
            raise NativeError("RunState: extra: present on one side only")

    def _shape_optimizers(self, manifest, host):
        """Optimiser state the snapshot lacks is dropped; state the live optimiser lacks is created (its contents are the unpack's to write); under a guard the
        parameters share step blocks as they did in the snapshot."""
        have = {e["name"] for e in manifest}
        for n, o in self._opts():
            info = host["optim"][n]
            guarded = info["guarded"]
            regroup = guarded and self._blocks_of(n, o) != list(info["blocks"])
            blocks = {}
            for i, p in enumerate(o.params):
                if f"optim.{n}.{i}.exp_avg" not in have:
                    o.state.pop(p, None)
                    continue
                s = o.state.get(p)
                if s is None:
                    s = o.state[p] = {"step": 0, "exp_avg": torch.empty_like(p.data), "exp_avg_sq": torch.empty_like(p.data)}
                if regroup:
                    b = info["blocks"][i]
                    if b not in blocks:
                        blocks[b] = torch.empty(16, dtype=torch.int32, device=p.device)
                    s["step_block"], s["step"] = blocks[b], blocks[b][0]

    def _set_host(self, host):
        from . import rng as R
        for n, o in self._opts():
            info = host["optim"][n]
            o.lr, o.betas, o.eps, o.weight_decay, o.grad_scale = float(info["lr"]), (float(info["betas"][0]), float(info["betas"][1])), float(info["eps"]), \
                float(info["weight_decay"]), float(info["grad_scale"])
            if not info["guarded"]:
                for p, step in zip(o.params, info["steps"]):
                    if step is not None:
                        o.state[p]["step"] = int(step)
        for g, d in zip(self._guards(), host["guards"]):
            for k in g.RULE:
                setattr(g, k, d[k])
            g.measurements = int(d["measurements"])
        for r, sd in zip(self._philox(), host["rngs"]):
            r.load_state_dict(sd)
            if r._fixed_seed is None and r._seed_seen is not None and r._seed_seen != torch.initial_seed():
                r._fixed_seed = r._seed_seen      # torch is seeded otherwise now: without the pin the next draw would start a new stream at counter 0
        if self.runner is not None:
            self.runner.iteration = int(host["iteration"])
        if self.sampler is not None:
            self.sampler.load_state_dict(host["sampler"])
        if self.ema is not None:
            self.ema.decay, self.ema.warmup = float(host["ema"]["decay"]), bool(host["ema"]["warmup"])
        for obj, d in ((self.augment, host["augment"]), (self.lecam, host["lecam"]), (self.spectral, host["spectral"])):
            if obj is not None:
                for k, v in d.items():
                    setattr(obj, k, v)
        if self.monitor is not None:
            self.monitor.interval, self.monitor.rolled = int(host["monitor"]["interval"]), int(host["monitor"]["rolled"])
        if self.extra is not None:
            self.extra.clear()
            self.extra.update(copy.deepcopy(host["extra"]))

    # ---- capture ------------------------------------------------------------------------------------------------------------------------------------------
    def _side_stream(self, device):
        if self._side is None:
            self._side = torch.cuda.Stream(device)
        return self._side

    def _workspace(self, lay: _Layout) -> torch.Tensor:
        need = int(lib().dcv_state_workspace_bytes(lay.n, lay.dwords))
        if need == 0:
            raise NativeError("dcv_state_workspace_bytes: " + lib().dcv_last_error().decode(errors="replace"))
        if self._ws is None or self._ws.numel() < need or self._ws.device != lay.device:
            self._ws = torch.empty(need, dtype=torch.uint8, device=lay.device)
        return self._ws

    def _ring(self, lay: _Layout):
        """All arenas of the ring and their digest tables, (re)allocated together when the layout changes: the steady state allocates nothing."""
        nbytes = max(lay.total * 4, 16)
        a0 = self._arenas[0]
        if a0 is None or a0.numel() != nbytes or a0.device != lay.device or self._digests[0].shape[0] != lay.n:
            for k in range(self.slots):
                self._arenas[k] = torch.empty(nbytes, dtype=torch.uint8, device=lay.device)
                self._digests[k] = torch.empty((lay.n, 2), dtype=torch.int64, device=lay.device)
                self._gen[k] += 1

    def capture(self) -> Snapshot:
        lay = self._layout()      # every refusal before the first launch
        self._ring(lay)
        slot = self._next % self.slots
        self._next += 1
        arena, digests = self._arenas[slot], self._digests[slot]
        if lay.device.type == "cuda":
            ws = self._workspace(lay)
            check(lib().dcv_state_pack_multi(lay.n, lay.src, lay.dwords, ptr(arena), lay.total, lay.offsets, ptr(digests), ptr(ws), ws.numel(), stream_ptr()),
                  "dcv_state_pack_multi")
        else:
            words = arena.numpy().view(np.uint32)
            words[:] = 0
            for k, (e, t) in enumerate(zip(lay.manifest, lay.tensors)):
                words[e["offset"]:e["offset"] + e["dwords"]] = _words(t)
                digests[k] = torch.tensor(_signed(digest_host(t)), dtype=torch.int64)
        self._gen[slot] += 1
        return Snapshot(self, [dict(e) for e in lay.manifest], self._host_scalars(), arena, digests, slot, self._gen[slot])

    # ---- files --------------------------------------------------------------------------------------------------------------------------------------------
    def load(self, path) -> Snapshot:
        """A snapshot from a file of ``Snapshot.save``.  The file's manifest is compared with the live objects' (NativeError naming the first entry that differs;
        nothing is written), the arena copied to the state's device and its segments' digests recomputed (a file whose bytes do not give its digests is refused,
        naming the entry).  ``restore()`` on the result applies it."""
        f = torch.load(path, map_location="cpu", weights_only=True)
        if not isinstance(f, dict) or f.get("format") != FORMAT_VERSION:
            raise NativeError(f"RunState.load: {path}: format {f.get('format') if isinstance(f, dict) else None!r}, this build reads {FORMAT_VERSION}")
        manifest = [dict(e, shape=tuple(e["shape"])) for e in f["manifest"]]
        host, h_arena, h_digests = f["host"], f["arena"], f["digests"]
        if h_arena.dtype != torch.uint8 or h_arena.dim() != 1 or h_digests.dtype != torch.int64 or tuple(h_digests.shape) != (len(manifest), 2):
            raise NativeError(f"RunState.load: {path}: the arena is a flat uint8 tensor and the digests (entries, 2) int64")
        total = _segments(manifest, h_arena.numel())
        h_words = h_arena.numpy().view(np.uint32)
        for e in manifest:      # the digests cover the segments; the (at most three) padding dwords behind each are zero by construction
            if h_words[e["offset"] + e["dwords"]:e["offset"] + _padded(e["dwords"])].any():
                raise NativeError(f"RunState.load: {path}: entry {e['name']}: the padding behind it is not zero — the file is damaged")
        self._check(manifest, host)
        device = self._layout().device
        stored = h_digests.tolist()
        if device.type == "cuda":
            arena = h_arena.to(device)
            digests = torch.empty((len(manifest), 2), dtype=torch.int64, device=device)
            dwords = c_array([e["dwords"] for e in manifest], C.c_int64)
            src = c_array([arena.data_ptr() + 4 * e["offset"] for e in manifest])
            ws = torch.empty(max(int(lib().dcv_state_workspace_bytes(len(manifest), dwords)), 16), dtype=torch.uint8, device=device)
            check(lib().dcv_state_digest_multi(len(manifest), src, dwords, ptr(digests), ptr(ws), ws.numel(), stream_ptr()), "dcv_state_digest_multi")
            found = digests.cpu().tolist()
        else:
            arena = h_arena.clone()
            words = arena.numpy().view(np.uint32)
            found = [_signed(digest_host(words[e["offset"]:e["offset"] + e["dwords"]])) for e in manifest]
            digests = torch.tensor(found, dtype=torch.int64).reshape(len(manifest), 2)
        for e, a, b in zip(manifest, stored, found):
            if list(a) != list(b):
                raise NativeError(f"RunState.load: {path}: entry {e['name']}: the arena's bytes give the digest {tuple(b)}, the file records {tuple(a)} — the file is damaged")
        assert total * 4 == arena.numel() or total == 0
        return Snapshot(self, manifest, host, arena, digests, None)

    # ---- fingerprint --------------------------------------------------------------------------------------------------------------------------------------
    def fingerprint(self) -> torch.Tensor:
        """(n_entries, 2) int64 on the state's device: the digests of the LIVE tensors, in manifest order.  No copy of the state, no host read; the table is this
        object's own and the next call overwrites it."""
        lay = self._layout()
        if self._fp is None or self._fp.shape[0] != lay.n or self._fp.device != lay.device:
            self._fp = torch.empty((lay.n, 2), dtype=torch.int64, device=lay.device)
        if lay.device.type == "cuda":
            ws = self._workspace(lay)
            check(lib().dcv_state_digest_multi(lay.n, lay.src, lay.dwords, ptr(self._fp), ptr(ws), ws.numel(), stream_ptr()), "dcv_state_digest_multi")
        else:
            for k, t in enumerate(lay.tensors):
                self._fp[k] = torch.tensor(_signed(digest_host(t)), dtype=torch.int64)
        return self._fp

    def fingerprint_host(self) -> "OrderedDict[str, Tuple[int, int]]":
        """name -> (sum, xor) of every entry, read back to the host."""
        lay = self._layout()
        rows = self.fingerprint().cpu().tolist()
        return OrderedDict((n, (int(r[0]), int(r[1]))) for n, r in zip(lay.names, rows))

    @staticmethod
    def diff(a, b) -> List[str]:
        """The names of the entries whose digests differ between two ``fingerprint_host()`` results (an entry one side lacks differs), in order."""
        return [n for n in list(a) + [m for m in b if m not in a] if a.get(n) != b.get(n)]


def model_state_dict(path, name: str) -> "OrderedDict[str, torch.Tensor]":
    """A reference-format CPU ``state_dict`` of one model (``"ggen"``) or of its EMA twin (``"ema.ggen"``), cut out of a file of ``Snapshot.save``: what
    ``sampling.load_model`` / ``load_state_dict`` take."""
    f = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(f, dict) or f.get("format") != FORMAT_VERSION:
        raise NativeError(f"runstate.model_state_dict: {path}: not a RunState file of format {FORMAT_VERSION}")
    prefix = (name if name.startswith("ema.") else "model." + name) + "."
    arena = f["arena"]
    _segments(f["manifest"], arena.numel())
    out = OrderedDict()
    for e in f["manifest"]:
        if e["name"].startswith(prefix):
            seg = arena[4 * e["offset"]:4 * (e["offset"] + e["dwords"])].clone()
            out[e["name"][len(prefix):]] = seg.view(_DTYPES[e["dtype"]]).reshape(tuple(e["shape"]))
    if not out:
        raise NativeError(f"runstate.model_state_dict: {path} holds no entry of {name!r}")
    return out
