"""Adam on the HIP kernel, and the data-parallel optimiser wrapper.

``Adam`` has torch.optim.Adam's semantics for the reference's wiring
(train.py:171-176: betas (0.5, 0.999), eps 1e-8, L2 weight decay): parameters
whose ``.grad`` is None are skipped, bias correction uses the per-optimiser step
count.  Only ``.step()`` / ``.zero_grad()`` are needed by a DCVGAN trainer.

``DataParallelAdam`` wraps an ``Adam`` for data-parallel training without any
trainer change: optimisers that are stepped after the same
backward share a ``GradBucket`` (D phase: idis + vdis + gdis, 15.9 MB; G phase:
ggen + cgen, 55.1 MB).  The first ``.step()`` after a backward all-reduces (sum)
the whole bucket — ONE collective per phase, two per iteration — and every
member's Adam kernel applies the 1/world factor as ``grad_scale``.  "After a
backward" is explicit state: a post-accumulate-grad hook on every parameter marks
the bucket dirty, the reduction clears the mark — so the trainer's double
``opt_ggen.step()`` reduces once, and nothing depends on object ids or tensor
version counters.

``GradGuard`` (optional, off by default) gives the optimisers registered with it a global gradient norm, clipping, a
skip of non-finite steps and (dynamic) loss scaling without a host read: see its docstring.  ``Adam(guard=None)`` is the
unguarded code path, unchanged.
"""
from __future__ import annotations

import ctypes as C
from typing import Iterable, List, Optional

import torch

from .native import NativeError, PointerTable, _require, c_array, check, lib, ptr, stream_ptr


class GradGuard:
    """Global gradient norm, clipping, non-finite skip and loss scaling for the ``Adam`` optimisers registered with it (``Adam(..., guard=g)``), measured, decided
    and applied on the device: nothing here reads a value on the host or runs a torch kernel.

        loss.backward(guard.root(loss))      # the root cotangent IS the current loss scale (a 0-d device tensor)
        guard.measure()                      # where a torch trainer calls scaler.unscale_ / clip_grad_norm_: once per backward
        opt_a.step(); opt_b.step()           # every step on this measurement applies — or skips on — the same decision

    ``measure()`` reads every registered parameter's ``.grad`` once (dcv_grad_guard_measure) and leaves norm, clip coefficient, the factor Adam multiplies the
    gradients by, the skip flag and the next loss scale in ``state`` (layout: DCV_GUARD_* in include/dcvgan_hip.h).  The decision rule is torch's:
    ``clip_grad_norm_``'s coefficient min(1, max_norm / (norm + 1e-6)) and ``torch.amp.GradScaler``'s skip / backoff / growth, with one difference: finite gradients
    whose sum of squares overflows fp32 count as non-finite.  For data-parallel members the gradients are reduced first and the norm is that of the averaged gradient,
    so every rank decides the same from the same bits."""

    FIELDS = ("loss_scale", "growth_tracker", "grad_norm", "clip_coef", "factor", "skipped", "skipped_total", "nonfinite")

    def __init__(self, max_norm: Optional[float] = None, skip_nonfinite: bool = True, loss_scale: float = 1.0, dynamic: bool = False,
                 growth_factor: float = 2.0, backoff_factor: float = 0.5, growth_interval: int = 2000):
        import math
        if max_norm is not None and not (float(max_norm) > 0.0 and math.isfinite(float(max_norm))):
            raise ValueError(f"GradGuard: max_norm must be a positive finite number or None, got {max_norm!r}")
        if not (float(loss_scale) > 0.0 and math.isfinite(float(loss_scale))):
            raise ValueError(f"GradGuard: loss_scale must be positive and finite, got {loss_scale!r}")
        if not float(growth_factor) > 1.0:
            raise ValueError(f"GradGuard: growth_factor must be > 1, got {growth_factor!r}")
        if not 0.0 < float(backoff_factor) < 1.0:
            raise ValueError(f"GradGuard: backoff_factor must be in (0, 1), got {backoff_factor!r}")
        if int(growth_interval) != growth_interval or int(growth_interval) < 1:
            raise ValueError(f"GradGuard: growth_interval must be a positive integer, got {growth_interval!r}")
        self.max_norm = None if max_norm is None else float(max_norm)
        self.skip_nonfinite, self.dynamic = bool(skip_nonfinite), bool(dynamic)
        self.init_scale = float(loss_scale)
        self.growth_factor, self.backoff_factor, self.growth_interval = float(growth_factor), float(backoff_factor), int(growth_interval)
        self.optimizers: List["Adam"] = []
        self._dp: List["DataParallelAdam"] = []
        self.state: Optional[torch.Tensor] = None
        self.measurements = 0
        self._ws: Optional[torch.Tensor] = None
        self._tables = None

    def _register(self, opt: "Adam"):
        self.optimizers.append(opt)
        dev = opt.params[0].device
        if self.state is None and dev.type == "cuda":      # (a host tensor -> device copy, once, before training: no kernel)
            self.state = torch.tensor([self.init_scale] + [0.0] * (len(self.FIELDS) - 1), dtype=torch.float32).to(dev)
        elif self.state is not None and dev != self.state.device:
            raise NativeError(f"GradGuard: optimisers on {self.state.device} and {dev} cannot share a guard")

    def _need_state(self) -> torch.Tensor:
        if self.state is None:
            raise NativeError("GradGuard: no optimiser with HIP device parameters is registered — the guard runs on the GPU only (there is no CPU fallback)")
        return self.state

    def root(self, loss: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The cotangent for ``loss.backward(...)``: the loss scale of this backward, a 0-d view of the device state."""
        return self._need_state()[0]

    def stats(self):
        """0-d device views of the state (they follow the next ``measure()``; copy what has to outlive it)."""
        s = self._need_state()
        return {k: s[self.FIELDS.index(k)] for k in ("grad_norm", "clip_coef", "skipped", "skipped_total", "loss_scale", "nonfinite")}

    RULE = ("max_norm", "skip_nonfinite", "dynamic", "init_scale", "growth_factor", "backoff_factor", "growth_interval")

    def state_dict(self):
        """The eight device floats (a host read: on request only; None while no optimiser with device parameters is registered), the number of measurements and
        the rule's constants."""
        sd = {k: getattr(self, k) for k in self.RULE}
        sd.update(state=None if self.state is None else self.state.detach().cpu().clone(), measurements=self.measurements)
        return sd

    @torch.no_grad()
    def load_state_dict(self, sd):
        st = sd["state"]
        if st is not None:
            if self.state is None:
                raise NativeError("GradGuard.load_state_dict: the checkpoint carries device state, but no optimiser with HIP device parameters is registered")
            if st.dtype != torch.float32 or st.numel() != len(self.FIELDS):
                raise ValueError(f"GradGuard.load_state_dict: the state is {len(self.FIELDS)} float32 values, the checkpoint holds {st.dtype} x {st.numel()}")
            self.state.copy_(st.reshape(-1))      # (host -> device: a copy, no kernel)
        self.max_norm = None if sd["max_norm"] is None else float(sd["max_norm"])
        self.skip_nonfinite, self.dynamic, self.init_scale = bool(sd["skip_nonfinite"]), bool(sd["dynamic"]), float(sd["init_scale"])
        self.growth_factor, self.backoff_factor, self.growth_interval = float(sd["growth_factor"]), float(sd["backoff_factor"]), int(sd["growth_interval"])
        self.measurements = int(sd["measurements"])

    @torch.no_grad()
    def measure(self):
        state = self._need_state()
        for w in self._dp:                   # data parallel: the norm of the REDUCED gradient (no-op when the bucket is clean)
            w.reduce_gradients()
            w.inner.grad_scale = 1.0 / w.world
        scales = {o.grad_scale for o in self.optimizers}
        if len(scales) != 1:
            raise NativeError(f"GradGuard: the registered optimisers disagree on grad_scale ({sorted(scales)})")
        gs, ns, keep = [], [], []
        for o in self.optimizers:
            for p in o.params:
                g = p.grad
                if g is None or g.numel() == 0:
                    continue
                _require(g, "GradGuard gradient")
                g = g.contiguous()
                gs.append(g.data_ptr()); ns.append(g.numel()); keep.append(g)
        tab = self._tables = PointerTable.cached(self._tables, (tuple(gs), tuple(ns)),
                                                 lambda: dict(n=len(gs), g=c_array(gs), numel=c_array(ns, C.c_int64)))
        L = lib()
        need = L.dcv_grad_guard_workspace_bytes(sum(ns), tab.n)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=state.device)
        check(L.dcv_grad_guard_measure(tab.n, tab.g, tab.numel, scales.pop(), self.max_norm if self.max_norm is not None else 0.0, int(self.skip_nonfinite), int(self.dynamic),
                                       self.growth_factor, self.backoff_factor, self.growth_interval, ptr(state), ptr(self._ws), self._ws.numel(), stream_ptr()),
              "dcv_grad_guard_measure")
        self.measurements += 1


class Adam:
    def __init__(self, params: Iterable[torch.nn.Parameter], lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                 guard: Optional[GradGuard] = None):
        self.params: List[torch.nn.Parameter] = [p for p in params]
        if not self.params:
            raise ValueError("optimizer got an empty parameter list")
        self.lr, self.betas, self.eps, self.weight_decay = float(lr), (float(betas[0]), float(betas[1])), float(eps), float(weight_decay)
        self.state = {}
        self.grad_scale = 1.0
        self.guard = guard
        if guard is not None:
            guard._register(self)

    def zero_grad(self, set_to_none: bool = True):
        for p in self.params:
            if set_to_none:
                p.grad = None
            elif p.grad is not None:
                p.grad.zero_()

    def state_dict(self):
        """torch.optim.Adam's layout — ``{"state": {index: {"step", "exp_avg", "exp_avg_sq"}}, "param_groups": [one group]}``, ``step`` a 0-d float32 host tensor —
        so that a ``torch.optim.Adam`` over the same parameters loads it, and this class loads torch's.  The moments are clones on the parameters' device.  Under a
        guard the step counts are read from the device blocks (a host read: on request only)."""
        state = {}
        for i, p in enumerate(self.params):
            s = self.state.get(p)
            if s is None:
                continue
            step = int(s["step"].item()) if isinstance(s["step"], torch.Tensor) else int(s["step"])
            state[i] = {"step": torch.tensor(float(step), dtype=torch.float32), "exp_avg": s["exp_avg"].detach().clone(), "exp_avg_sq": s["exp_avg_sq"].detach().clone()}
        group = {"lr": self.lr, "betas": self.betas, "eps": self.eps, "weight_decay": self.weight_decay, "amsgrad": False, "maximize": False, "foreach": None,
                 "capturable": False, "differentiable": False, "fused": None, "decoupled_weight_decay": False, "params": list(range(len(self.params)))}
        return {"state": state, "param_groups": [group]}

    @torch.no_grad()
    def load_state_dict(self, sd):
        """The inverse, also of ``torch.optim.Adam.state_dict()``: one parameter group over the same parameters in the same order, no amsgrad, no maximize.  State
        of parameters the checkpoint does not list is dropped.  Under a guard, parameters with the same step count share one device step block.  Every refusal
        comes before anything is changed."""
        groups = sd["param_groups"]
        if len(groups) != 1 or list(groups[0]["params"]) != list(range(len(self.params))):
            raise ValueError(f"Adam.load_state_dict: expected one parameter group over {len(self.params)} parameters, got "
                             f"{[len(g['params']) for g in groups]}")
        g = groups[0]
        if g.get("amsgrad") or g.get("maximize") or g.get("decoupled_weight_decay"):
            raise ValueError("Adam.load_state_dict: amsgrad / maximize / decoupled weight decay checkpoints have no counterpart here")
        new = {}
        for i, st in sd["state"].items():
            i = int(i)
            if not 0 <= i < len(self.params):
                raise ValueError(f"Adam.load_state_dict: state of parameter {i} of {len(self.params)}")
            p = self.params[i]
            for k in ("exp_avg", "exp_avg_sq"):
                if tuple(st[k].shape) != tuple(p.shape):
                    raise ValueError(f"Adam.load_state_dict: {k} of parameter {i} is {tuple(st[k].shape)}, the parameter {tuple(p.shape)}")
            step = float(st["step"])
            if step != int(step) or step < 0:
                raise ValueError(f"Adam.load_state_dict: step {step!r} of parameter {i}")
            new[i] = (int(step), st["exp_avg"], st["exp_avg_sq"])
        self.lr, self.betas, self.eps, self.weight_decay = float(g["lr"]), (float(g["betas"][0]), float(g["betas"][1])), float(g["eps"]), float(g["weight_decay"])
        self.state = {}
        blocks = {}
        for i, (step, m, v) in new.items():
            p = self.params[i]
            s = self.state[p] = {"step": step, "exp_avg": torch.empty_like(p.data).copy_(m), "exp_avg_sq": torch.empty_like(p.data).copy_(v)}
            if self.guard is not None:      # (host tensor -> device copy: no kernel)
                key = (step, p.device)
                if key not in blocks:
                    blocks[key] = torch.tensor([step] + [0] * 15, dtype=torch.int32).to(p.device)
                s["step_block"], s["step"] = blocks[key], blocks[key][0]

    def _step_guarded(self):
        """The step under a GradGuard: the step count lives on the device (a skipped step must not advance it, and the host does not know), one 64-byte step block
        per set of parameters that started together — ``state[p]["step"]`` is its first word — and one dcv_adam_step_multi_guarded call per block."""
        guard = self.guard
        if guard.measurements == 0:
            raise NativeError("Adam(guard=...): step() before any guard.measure() — there is no decision to apply")
        L = lib()
        st = stream_ptr()
        groups, touched, fresh = {}, [], None
        for p in self.params:
            g = p.grad
            if g is None:
                continue
            _require(p.data, "Adam parameter")
            if not p.data.is_contiguous():
                raise NativeError("Adam: parameters must be contiguous")
            g = g.contiguous()
            s = self.state.get(p)
            if s is None:
                if fresh is None:
                    fresh = torch.zeros(16, dtype=torch.int32, device=p.device)      # DCV_ADAM_STEP_BLOCK_BYTES
                s = self.state[p] = {"step": fresh[0], "step_block": fresh, "exp_avg": torch.zeros_like(p.data), "exp_avg_sq": torch.zeros_like(p.data)}
            touched.append(p)
            grp = groups.setdefault(s["step_block"].data_ptr(), ([], [], [], [], [], []))
            grp[0].append(p.data.data_ptr()); grp[1].append(g.data_ptr()); grp[2].append(s["exp_avg"].data_ptr()); grp[3].append(s["exp_avg_sq"].data_ptr())
            grp[4].append(p.numel()); grp[5].append(g)
        for block, (ps, gs, ms, vs, ns, _) in groups.items():
            check(L.dcv_adam_step_multi_guarded(len(ps), c_array(ps), c_array(gs), c_array(ms), c_array(vs), c_array(ns, C.c_int64), self.lr, self.betas[0], self.betas[1],
                                                self.eps, self.weight_decay, C.c_void_p(block), ptr(guard.state), st), "dcv_adam_step_multi_guarded")
        if touched:
            torch.autograd.graph.increment_version(touched)

    @torch.no_grad()
    def step(self):
        if self.guard is not None:
            return self._step_guarded()
        L = lib()
        st = stream_ptr()
        ps, gs, ms, vs, ns, keep = [], [], [], [], [], []
        touched = []
        step = None
        for p in self.params:
            g = p.grad
            if g is None:
                continue
            _require(p.data, "Adam parameter")
            if not p.data.is_contiguous():
                raise NativeError("Adam: parameters must be contiguous")
            g = g.contiguous()
            s = self.state.get(p)
            if s is None:
                s = self.state[p] = {"step": 0, "exp_avg": torch.zeros_like(p.data), "exp_avg_sq": torch.zeros_like(p.data)}
            s["step"] += 1
            touched.append(p)
            if step is None:
                step = s["step"]
            if s["step"] != step:   # parameters that joined later keep their own bias correction: single-tensor path
                check(L.dcv_adam_step(ptr(p.data), ptr(g), ptr(s["exp_avg"]), ptr(s["exp_avg_sq"]), p.numel(), self.lr, self.betas[0], self.betas[1],
                                      self.eps, self.weight_decay, s["step"], self.grad_scale, st), "dcv_adam_step")
                continue
            ps.append(p.data.data_ptr()); gs.append(g.data_ptr()); ms.append(s["exp_avg"].data_ptr()); vs.append(s["exp_avg_sq"].data_ptr())
            ns.append(p.numel()); keep.append(g)
        if ps:
            check(L.dcv_adam_step_multi(len(ps), c_array(ps), c_array(gs), c_array(ms), c_array(vs), c_array(ns, C.c_int64), self.lr, self.betas[0], self.betas[1],
                                        self.eps, self.weight_decay, step, self.grad_scale, st), "dcv_adam_step_multi")
        if touched:
            # the kernels wrote through raw pointers: tell autograd (and the packed-weight caches keyed on it) that
            # these tensors changed in place
            torch.autograd.graph.increment_version(touched)


class ModelEma:
    """Exponential moving averages of the generators' weights — the twins a GAN is sampled and evaluated from — kept on the device.

        ema = ModelEma(models, names=("ggen", "cgen"), decay=0.999, warmup=True, guard=opt_ggen.guard)
        ema.update()                         # once per iteration in which the generators were stepped, after their last step
        sampling.generate_samples(ema.module("ggen"), ema.module("cgen"), ...)

    A twin is a deep copy of the live model (same class, same ``state_dict`` keys, its own storage), in eval mode, without gradients; the twins share one random
    stream (``ema.rng``) that is not the live models'.
    ``update()`` is one dcv_ema_update_multi call per model on the current stream: parameters e += (1 - d_t)(p - e) with d_t = min(decay, (1 + t) / (10 + t)) under
    ``warmup`` (t = updates applied so far, counted on the device), buffers (BatchNorm running statistics, num_batches_tracked) copied bit for bit.  With a
    ``guard`` the update applies — or skips on — the guard's last measurement, like the optimiser steps on it: a skipped update changes no tensor and no count.
    Nothing here reads a value on the host, runs a torch kernel or allocates in the steady state.  GPU only: ``update()`` on CPU models, non-fp32 or
    non-contiguous parameters raises ``NativeError`` before any launch."""

    def __init__(self, models, names=("ggen", "cgen"), decay: float = 0.999, warmup: bool = True, guard: Optional[GradGuard] = None):
        if not 0.0 <= float(decay) < 1.0:
            raise ValueError(f"ModelEma: decay must be in [0, 1), got {decay!r}")
        self.names = tuple(names)
        if not self.names:
            raise ValueError("ModelEma: no model names")
        self.decay, self.warmup, self.guard = float(decay), bool(warmup), guard
        from .rng import PhiloxRng
        self.live = {n: models[n] for n in self.names}
        # ONE random stream for all twins, apart from the live models': a PhiloxRng is (seed, counter), so two of them would hand two twins the same values, and the
        # colour twin's latent would repeat the geometry twin's.  On one stream the twins' draws interleave, as the live models' do on rng.default_rng().
        self.rng = PhiloxRng()
        self.twins = {n: self._twin(m, self.rng) for n, m in self.live.items()}
        # (twin tensor, live tensor) in state_dict order, parameters first
        self._pairs = {}
        for n, m in self.live.items():
            tp, tb = dict(self.twins[n].named_parameters()), dict(self.twins[n].named_buffers())
            self._pairs[n] = [(tp[k], p) for k, p in m.named_parameters()] + [(tb[k], b) for k, b in m.named_buffers()]
        self._n_params = {n: sum(1 for _ in m.parameters()) for n, m in self.live.items()}
        self._tables = {}
        dev = next(self.live[self.names[0]].parameters()).device
        # per model: DCV_EMA_BLOCK_BYTES beside the models; word 0 is the number of updates applied (host tensor -> device copies, once: no kernel).  Host models get
        # a host block: update() refuses them, but a checkpoint's count still loads and reads back.
        self._blocks = {n: torch.zeros(16, dtype=torch.int32).to(dev) for n in self.names}

    @staticmethod
    def _twin(model: torch.nn.Module, twin_rng) -> torch.nn.Module:
        import copy
        rng = model.__dict__.pop("_rng", None)      # the live model's random source is not copied: the twins draw from the ModelEma's own stream
        try:
            twin = copy.deepcopy(model)
        finally:
            model.__dict__["_rng"] = rng
        twin._rng = twin_rng
        for t in list(twin.parameters()) + list(twin.buffers()):      # nothing cached for the live tensors (packed weights, bucket slices) may follow the copy
            for k in [k for k in t.__dict__ if k.startswith("_dcv_")]:
                del t.__dict__[k]
        for p in twin.parameters():
            p.requires_grad_(False)
        return twin.eval()

    def module(self, name: str) -> torch.nn.Module:
        return self.twins[name]

    def _table(self, name: str) -> PointerTable:
        key = tuple(t.data_ptr() for pair in self._pairs[name] for t in pair)
        tab = self._tables[name] = PointerTable.cached(self._tables.get(name), key, lambda: self._build_table(name))
        return tab

    def _build_table(self, name: str) -> dict:
        pairs = self._pairs[name]
        es, ss, ns, ms = [], [], [], []
        for i, (e, s) in enumerate(pairs):
            what = f"ModelEma({name}) " + ("parameter" if i < self._n_params[name] else "buffer")
            for t in (e, s):
                if not t.is_cuda:
                    raise NativeError(f"{what}: expected a HIP device tensor, got {t.device} — the EMA runs on the GPU only (there is no CPU fallback)")
                if t.device.index != torch.cuda.current_device():
                    raise NativeError(f"{what}: tensor is on {t.device} but the current device is cuda:{torch.cuda.current_device()}")
                if not t.is_contiguous():
                    raise NativeError(f"{what}: tensors must be contiguous")
            if e.dtype != s.dtype or e.shape != s.shape:
                raise NativeError(f"{what}: the twin holds {e.dtype}{tuple(e.shape)}, the live model {s.dtype}{tuple(s.shape)}")
            if i < self._n_params[name]:
                if s.dtype != torch.float32:
                    raise NativeError(f"{what}: expected float32, got {s.dtype}")
                mode, dwords = 0, s.numel()
            else:
                if s.element_size() % 4:
                    raise NativeError(f"{what}: buffers are copied as 32-bit words, got {s.dtype}")
                mode, dwords = 1, s.numel() * (s.element_size() // 4)
            if dwords == 0:
                continue
            es.append(e.data_ptr()); ss.append(s.data_ptr()); ns.append(dwords); ms.append(mode)
        return dict(n=len(es), ema=c_array(es), src=c_array(ss), numel=c_array(ns, C.c_int64), mode=c_array(ms, C.c_int32), touched=[e for e, _ in pairs])

    @torch.no_grad()
    def update(self):
        tabs = [self._table(n) for n in self.names]      # every refusal before the first launch
        state = ptr(self.guard._need_state()) if self.guard is not None else None
        L = lib()
        st = stream_ptr()
        for name, t in zip(self.names, tabs):
            check(L.dcv_ema_update_multi(t.n, t.ema, t.src, t.numel, t.mode, self.decay, int(self.warmup), ptr(self._blocks[name]), state, st), "dcv_ema_update_multi")
            # the kernels wrote through raw pointers: the twin's packed-weight caches are keyed on the version counter, as in Adam.step (harmless after a skipped update)
            torch.autograd.graph.increment_version(t.touched)

    def num_updates(self) -> int:
        """Updates applied so far (a host read of the device count: on request only)."""
        counts = {int(b[0].item()) for b in self._blocks.values()}
        if len(counts) > 1:
            raise NativeError(f"ModelEma: the models' update counts differ ({sorted(counts)})")
        return counts.pop() if counts else 0

    def _set_count(self, count: int):
        for b in self._blocks.values():
            b.copy_(torch.tensor([int(count)] + [0] * 15, dtype=torch.int32))

    def state_dict(self):
        """Per model an ordinary checkpoint of the twin (reference format), plus the count and the rule."""
        sd = {n: self.twins[n].state_dict() for n in self.names}
        sd.update(num_updates=self.num_updates(), decay=self.decay, warmup=self.warmup)
        return sd

    @torch.no_grad()
    def load_state_dict(self, sd):
        for n in self.names:
            self.twins[n].load_state_dict(sd[n])
        self.decay, self.warmup = float(sd["decay"]), bool(sd["warmup"])
        self._set_count(sd["num_updates"])

    @torch.no_grad()
    def reset(self):
        """twins := live models, count := 0."""
        for pairs in self._pairs.values():
            for e, s in pairs:
                e.copy_(s)
        self._set_count(0)


def _copy_into(slot: torch.Tensor, g: torch.Tensor) -> None:
    """slot <- g with the library's strided copy (dcv_axpby) on the device; torch's copy on the host (gloo rehearsals)."""
    if slot.is_cuda and g.dtype == torch.float32 and g.dim() in (2, 4, 5):
        from . import ops
        ops._axpby(g, 1.0, None, 0.0, slot)
    elif slot.is_cuda and g.dtype == torch.float32:
        from . import ops
        ops._axpby(g.reshape(1, -1) if g.is_contiguous() else g.contiguous().reshape(1, -1), 1.0, None, 0.0, slot.reshape(1, -1))
    else:
        slot.copy_(g)


def _zero_slot(p) -> None:
    """p's gradient slice <- 0.  On the device: 0 * p (the parameter is finite where the stale slice need not be) through dcv_axpby, so that no torch fill
    kernel runs beside the library's (DESIGN: packed-FP32 code of torch's elementwise kernels is outside the build's control)."""
    slot = p._dcv_grad_slot
    if slot.is_cuda:
        from . import ops
        ops._axpby(p.detach().reshape(1, -1), 0.0, None, 0.0, slot.reshape(1, -1))
    else:
        slot.zero_()


class GradBucket:
    """The gradients that one backward produces and one group of optimiser steps consumes.

    Round 4: the bucket owns ONE persistent flat fp32 buffer (allocated at the first reduction, sized for all members) and every
    member's ``.grad`` IS its slice of it: the post-accumulate-grad hook — which also marks the bucket dirty — re-points ``p.grad`` at
    the slice (copying only when the gradient was produced elsewhere; the weight-gradient kernels write straight into the slice,
    ``ops._Conv.backward``).  ``reduce()`` is then in-place all-reduces (sum) of the buffer — no flatten copy, no re-pointing afterwards.  The slice of a parameter
    whose ``.grad`` is None this backward (the set is the same on every rank: every rank runs the same graph) is zeroed before the collective:
    nobody reads it, but a stale slice would be multiplied by the world size at every reduction and reach inf / NaN inside the communicated
    buffer (RCCL's NaN checks, anomaly tooling).
    `dirty` is set by autograd whenever a member receives a gradient and cleared by `reduce()`.

    Round 5, ``overlap=True``: the buffer is cut into CHUNKS — one per ``add()`` call, i.e. per model (small neighbours merged up to ``merge_bytes``, large ones cut at
    ``bucket_bytes``) — and a chunk's collective is launched from the hook of the LAST gradient of that chunk to land, on a communication stream behind the events of
    the streams that produced the chunk's gradients, while the backward of the other models is still running (G phase: cgen's 40 MB are reduced under ggen's backward);
    ``reduce()`` then only waits.  Which gradient is a chunk's last one is LEARNED: the set and order of arrivals of the previous backward of this bucket (the same graph
    every iteration); a backward whose arrivals differ from the record simply is not overlapped (the step reduces synchronously, chunk by chunk — the same collectives on
    the same ranges, so both ways give the same bits).  Safety: a chunk is only launched early when none of its members held a gradient at the start of this backward; a
    gradient that arrives for a chunk that is already in flight, or is added in place to it (``ops.grad_target``) before the step has consumed it, raises; the weight-gradient
    op orders itself behind a collective still reading the slice it is about to overwrite (``before_slot_write``)."""

    def __init__(self, group=None, bucket_bytes: int = 256 << 20, overlap: bool = False, merge_bytes: int = 4 << 20):
        import torch.distributed as dist
        self.dist, self.group = dist, group
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        self.bucket_bytes, self.merge_bytes, self.overlap = bucket_bytes, merge_bytes, bool(overlap)
        self.params: List[torch.nn.Parameter] = []
        self.dirty = False
        self.collectives = 0      # counters for tests / bench
        self.reductions = 0
        self.copies = 0           # gradients that had to be copied into their slice (produced outside it)
        self.early = 0            # collectives launched from a hook, during the backward
        self._hooks = []
        self._groups = []         # member lists, one per add()
        self._flat: Optional[torch.Tensor] = None
        self._chunks = []         # _Chunk objects: element ranges of the buffer, one collective each
        self._comm = None
        self.timed = None         # a list: (start event, end event, bytes) of every collective launched from reduce() (bench.py's per-phase collective time)

    class _Chunk:
        __slots__ = ("a", "b", "members", "record", "arrived", "events", "work", "task", "fresh")

        def __init__(self, a, b, members):
            self.a, self.b, self.members = a, b, members
            self.record = None        # (frozenset of member ids that received a gradient, id of the last one to arrive) in the previous backward
            self.arrived, self.events, self.work, self.task, self.fresh = [], [], None, -2, True

    def _layout(self):
        """Allocate the flat buffer, hand every member its slice (`p._dcv_grad_slot`, read by the weight-gradient ops) and cut the chunks."""
        p0 = self.params[0]
        total = 0
        spans = []                # (first element, one past the last, members) per add() group
        groups = self._groups if (self.overlap and self._groups) else [self.params]      # without overlap the bucket is ONE message (cut only at bucket_bytes)
        for members in groups:
            g0 = total
            for p in members:
                if p.dtype != torch.float32:
                    raise NativeError("GradBucket: fp32 parameters only")
                p._dcv_grad_off = total
                total += (p.numel() + 63) // 64 * 64      # slices start on 256-byte boundaries (16-byte stores of the reduce kernels)
            spans.append((g0, total, list(members)))
        # chunks: small neighbouring groups merged, a group beyond bucket_bytes cut at member boundaries
        self._chunks = []
        cur_a, cur_members = 0, []
        for (a, b, members) in spans:
            cur_end = cur_members[-1]._dcv_grad_off + (cur_members[-1].numel() + 63) // 64 * 64 if cur_members else cur_a      # one past the open chunk's last member
            if cur_members and ((b - cur_a) * 4 > self.bucket_bytes or ((cur_end - cur_a) * 4 >= self.merge_bytes and (b - a) * 4 >= self.merge_bytes)):
                self._chunks.append(GradBucket._Chunk(cur_a, a, cur_members))
                cur_a, cur_members = a, []
            for p in members:
                if cur_members and (p._dcv_grad_off + (p.numel() + 63) // 64 * 64 - cur_a) * 4 > self.bucket_bytes:
                    self._chunks.append(GradBucket._Chunk(cur_a, p._dcv_grad_off, cur_members))
                    cur_a, cur_members = p._dcv_grad_off, []
                cur_members.append(p)
        if cur_members:
            self._chunks.append(GradBucket._Chunk(cur_a, total, cur_members))
        self._flat = torch.zeros(total, dtype=torch.float32, device=p0.device)
        for c in self._chunks:
            for p in c.members:
                p._dcv_grad_slot = self._flat[p._dcv_grad_off:p._dcv_grad_off + p.numel()].view(p.shape)
                p._dcv_chunk = c

    def _mark(self, p):
        self.dirty = True
        if self.world == 1 and not self._force_layout:
            return
        if self._flat is None or self._flat.device != p.device:
            self._layout()
        g, slot = p.grad, p._dcv_grad_slot
        if g is not None and g.data_ptr() != slot.data_ptr():
            _copy_into(slot, g)
            p.grad = slot
            self.copies += 1
        if self.overlap:
            self._arrival(p)

    _force_layout = False

    # ---- overlap ------------------------------------------------------------------------------------------------------------------
    def _arrival(self, p):
        c = p._dcv_chunk
        task = torch._C._current_graph_task_id()
        if c.task != task:                      # first gradient of this chunk in a new backward
            if c.work is not None:
                raise NativeError("GradBucket(overlap=True): a new backward delivers gradients to a chunk whose collective of the previous backward has not been "
                                  "consumed by an optimiser step (gradient accumulation over several backwards needs overlap=False)")
            c.task, c.arrived, c.events = task, [], []
            # early launch only for a backward that STARTS from empty gradients (zero_grad before it): at the first arrival every other member must still be without one
            c.fresh = all(q.grad is None for q in c.members if q is not p)
        elif c.work is not None:
            raise NativeError("GradBucket(overlap=True): a gradient arrived for a chunk that is already being reduced (the arrival order changed between backwards)")
        c.arrived.append(id(p))
        if p.is_cuda:
            e = torch.cuda.Event()
            e.record(torch.cuda.current_stream(p.device))
            c.events.append(e)
        rec = c.record
        if rec is not None and id(p) == rec[1] and len(c.arrived) == len(rec[0]) and frozenset(c.arrived) == rec[0] and c.fresh \
                and all(q.grad is None for q in c.members if id(q) not in rec[0]):      # (a member that keeps an old gradient and gets none now would be summed again)
            self._launch(c, early=True)

    def note_inplace(self, p):
        """ops.grad_target adds a gradient to p.grad in place (no AccumulateGrad visit, no hook): the bucket is dirty; a chunk that was reduced early and not consumed yet
        must not be added to, and a chunk that receives in-place additions is not 'fresh' (its collective waits for the step)."""
        self.dirty = True
        c = getattr(p, "_dcv_chunk", None)
        if c is None:
            return
        if c.work is not None:
            raise NativeError("GradBucket(overlap=True): a gradient is being added in place to a chunk whose early collective has not been consumed by an optimiser step")
        c.fresh = False

    def before_slot_write(self, p):
        """The weight-gradient op is about to write p's slice: order the current stream behind a collective that is still reading it."""
        c = getattr(p, "_dcv_chunk", None)
        if c is not None and c.work is not None and p.is_cuda:
            c.work.wait()

    def _launch(self, c, early):
        flat = self._flat
        if flat.is_cuda:
            if self._comm is None:
                self._comm = torch.cuda.Stream(flat.device)
            cur = torch.cuda.current_stream(flat.device)
            if early:
                with torch.cuda.stream(self._comm):
                    for e in c.events:
                        self._comm.wait_event(e)
                    for q in c.members:          # slices of members without a gradient this backward: zeroed before they are summed over the ranks
                        if q.grad is None:
                            _zero_slot(q)
                    c.work = self.dist.all_reduce(flat[c.a:c.b], op=self.dist.ReduceOp.SUM, group=self.group, async_op=True)
                flat.record_stream(self._comm)
            else:
                if self.timed is not None:      # bench.py: HIP events around the collective as the compute stream sees it (issue ... data reduced)
                    e0 = torch.cuda.Event(enable_timing=True); e0.record(cur)
                c.work = self.dist.all_reduce(flat[c.a:c.b], op=self.dist.ReduceOp.SUM, group=self.group, async_op=True)
                if self.timed is not None:
                    c.work.wait()
                    e1 = torch.cuda.Event(enable_timing=True); e1.record(cur)
                    self.timed.append((e0, e1, (c.b - c.a) * 4))
        else:
            self.dist.all_reduce(flat[c.a:c.b], op=self.dist.ReduceOp.SUM, group=self.group)
            c.work = True                        # CPU (gloo rehearsal): done on return
        self.collectives += 1
        if early:
            self.early += 1

    def add(self, params: Iterable[torch.nn.Parameter]):
        have = {id(p) for p in self.params}
        members = []
        for p in params:
            if id(p) in have:
                continue              # already a member (a wrapper built around a bucket that was filled by hand)
            self.params.append(p)
            members.append(p)
            import weakref
            p._dcv_bucket = weakref.ref(self)     # ops.grad_target marks the bucket dirty when it adds a gradient in place (no AccumulateGrad visit, no hook)
            self._hooks.append(p.register_post_accumulate_grad_hook(self._mark))
            self._flat = None         # a new member: the buffer is laid out again at the next gradient (existing .grad slices are copied over)
        if members:
            self._groups.append(members)

    @torch.no_grad()
    def reduce(self, force: bool = False):
        """`force`: run the collective even in a world of one (the RCCL smoke test pushes the real 55 MB bucket through the
        `nccl` backend on a single card this way)."""
        if not self.dirty:
            return
        self.dirty = False
        if self.world == 1 and not (force and self.dist.is_initialized()):
            return
        if self._flat is None:      # gradients arrived before the layout existed (world of one, force=True): adopt them now
            self._layout()
        self.reductions += 1
        for c in self._chunks:
            if c.work is None:      # not launched during the backward: now, on the current stream
                for p in c.members:
                    if p.grad is None:
                        _zero_slot(p)                 # no gradient this backward: the stale slice must not be summed over the ranks again and again
                    elif p.grad.data_ptr() != p._dcv_grad_slot.data_ptr():
                        _copy_into(p._dcv_grad_slot, p.grad)
                        p.grad = p._dcv_grad_slot
                        self.copies += 1
                self._launch(c, early=False)
        for c in self._chunks:      # the optimiser steps that follow read the reduced slices on the current stream
            if c.work is not None and c.work is not True:
                c.work.wait()
            # remember this backward's arrivals: the next backward of the same graph launches the chunk from its last arrival's hook
            c.record = (frozenset(c.arrived), c.arrived[-1]) if (self.overlap and c.arrived) else c.record
            c.work, c.arrived, c.events, c.task, c.fresh = None, [], [], -2, True
        from . import ops
        ops.new_backward_epoch()      # this backward's gradients are in the buffer: the weight-gradient ops may be handed the slices again (also when a plain Adam drives the bucket)


class DataParallelAdam:
    """Wraps an ``Adam``: reduce the shared bucket if a backward has run since the last reduction, then
    step with grad_scale = 1/world."""

    def __init__(self, inner: Adam, bucket: Optional[GradBucket] = None, group=None):
        self.inner = inner
        self.bucket = bucket if bucket is not None else GradBucket(group)
        self.bucket.add(inner.params)
        self.world = self.bucket.world
        if getattr(inner, "guard", None) is not None:      # guard.measure() reduces this wrapper's bucket first and measures the averaged gradient (grad_scale = 1 / world)
            inner.guard._dp.append(self)
            inner.grad_scale = 1.0 / self.world

    @property
    def params(self):
        return self.inner.params

    @property
    def guard(self):
        return getattr(self.inner, "guard", None)      # (the wrapper also drives optimisers that know no guard)

    def zero_grad(self, set_to_none: bool = True):
        self.inner.zero_grad(set_to_none)

    def reduce_gradients(self):
        self.bucket.reduce()

    def state_dict(self):
        return self.inner.state_dict()

    def load_state_dict(self, sd):
        self.inner.load_state_dict(sd)

    def step(self):
        self.bucket.reduce()
        self.inner.grad_scale = 1.0 / self.world
        self.inner.step()
        from . import ops
        ops.new_backward_epoch()      # this backward's gradients are consumed: the weight-gradient ops may write into the slices again


def broadcast_module(module: torch.nn.Module, src: int = 0, group=None):
    """Make every rank start from rank `src`'s parameters and buffers."""
    import torch.distributed as dist
    if not dist.is_initialized() or dist.get_world_size(group) == 1:
        return
    with torch.no_grad():
        ts = list(module.parameters()) + list(module.buffers())
        for t in ts:
            dist.broadcast(t.data, src, group=group)
        torch.autograd.graph.increment_version(ts)   # `.data` writes bypass the version counter


def broadcast_buffers(module: torch.nn.Module, src: int = 0, group=None):
    """BatchNorm running statistics stay per-rank during data-parallel training (each rank = one reference trainer);
    call this before a snapshot / evaluation (trainer.py:70-86, :196) when every rank should save rank `src`'s statistics."""
    import torch.distributed as dist
    if not dist.is_initialized() or dist.get_world_size(group) == 1:
        return
    with torch.no_grad():
        for b in module.buffers():
            dist.broadcast(b.data, src, group=group)


# --------------------------------------------------------------------------- #
# Synchronised BatchNorm (fp32 path)
# --------------------------------------------------------------------------- #
class SyncBnGroup:
    """The handle a marked BatchNorm module carries (`sync_batchnorm`): the ranks whose batches one BatchNorm group normalises together, and the exchange of their sums.

    One collective per BatchNorm group and pass: an all-reduce(SUM) of a zeroed (world, 2C + 1) fp64 table in which this rank has filled only its own row.  Adding
    zeros is exact, so this is an all-gather that gloo (on device tensors) and RCCL both have, and its result is the same table on every rank.  It is issued on the
    current stream, without a host read.  The process group is the handle's own (`dist.new_group`): these collectives never share a communicator with a gradient
    bucket's, plain or overlapped.  Every rank must run the same BatchNorm groups in the same host order — they do: every rank runs the same graph.
    `force`: run the sync kernels in a world of one too (no collective): the cost tool and single-process tests."""

    def __init__(self, ranks=None, force: bool = False, timeout=None):
        import torch.distributed as dist
        self.dist, self.force = dist, bool(force)
        self.pg, self.world, self.rank = None, 1, 0
        ranks = None if ranks is None else sorted(int(r) for r in ranks)
        if dist.is_initialized() and dist.get_world_size() > 1 and (ranks is None or len(ranks) > 1):
            ranks = ranks if ranks is not None else list(range(dist.get_world_size()))
            # (every rank of the default group has to make this call, members or not: torch.distributed's rule for new_group)
            self.pg = dist.new_group(ranks=ranks, **({"timeout": timeout} if timeout is not None else {}))
            if dist.get_rank() in ranks:
                self.world, self.rank = len(ranks), ranks.index(dist.get_rank())
            else:
                self.pg = None
        self.collectives = 0      # counter for tests / tools

    @property
    def active(self) -> bool:
        return self.world > 1 or self.force

    def table(self, channels: int, device) -> torch.Tensor:
        n = 2 * int(channels) + 1
        if self.world == 1:
            return torch.empty((1, n), dtype=torch.float64, device=device)      # the one row is written whole
        return torch.zeros((self.world, n), dtype=torch.float64, device=device)

    def exchange(self, rows: torch.Tensor) -> None:
        if self.world == 1:
            return
        self.dist.all_reduce(rows, op=self.dist.ReduceOp.SUM, group=self.pg)
        self.collectives += 1

    def __deepcopy__(self, memo):
        return self      # copies of a marked module (an EMA twin) exchange with the same ranks


def _batchnorms(module_or_models):
    mods = module_or_models.values() if isinstance(module_or_models, dict) else \
        [module_or_models] if isinstance(module_or_models, torch.nn.Module) else list(module_or_models)
    seen = set()
    for m in mods:
        for sub in m.modules():
            if isinstance(sub, (torch.nn.BatchNorm2d, torch.nn.BatchNorm3d)) and id(sub) not in seen:
                seen.add(id(sub))
                yield sub


def sync_batchnorm(module_or_models, group=None, force: bool = False) -> SyncBnGroup:
    """Mark every BatchNorm2d / BatchNorm3d of a module (or of a dict / sequence of modules) for synchronised statistics: in training mode, with more than one rank
    (or `force`), its statistics and its backward's reduction sums cover the batch of all ranks of `group` — the numerics of one process on the concatenated batch
    (DESIGN §7a).  fp32 path only.  `group`: None (all ranks), a sequence of global ranks, or a SyncBnGroup made earlier (to share one communicator between calls).
    Collective: every rank must call this (it makes a process group).  Returns the handle; `unsync_batchnorm` removes the marks."""
    handle = group if isinstance(group, SyncBnGroup) else SyncBnGroup(group, force=force)
    if isinstance(group, SyncBnGroup) and force:
        handle.force = True
    for bn in _batchnorms(module_or_models):
        bn._dcv_sync_bn = handle
    return handle


def unsync_batchnorm(module_or_models) -> None:
    """The inverse of `sync_batchnorm`: every BatchNorm of the module(s) keeps its statistics local again."""
    for bn in _batchnorms(module_or_models):
        bn.__dict__.pop("_dcv_sync_bn", None)


def sync_bn_group_of(module_or_models) -> Optional[SyncBnGroup]:
    """The handle of the first marked BatchNorm of the module(s), or None when nothing is marked."""
    for bn in _batchnorms(module_or_models):
        h = bn.__dict__.get("_dcv_sync_bn")
        if h is not None:
            return h
    return None


# --------------------------------------------------------------------------- #
# Spectral normalisation of the discriminators' convolutions (fp32 path)
# --------------------------------------------------------------------------- #
class _SpectralMark:
    """What a marked convolution carries in ``__dict__["_dcv_spectral"]``: W / sigma (plain device memory, not a buffer: it is recomputed, never saved) and the
    autograd version of the weight it was computed from.  A deep copy of the module gets None in its place: the copy carries the buffers and no mark."""
    __slots__ = ("w_sn", "version")

    def __init__(self, w_sn):
        self.w_sn, self.version = w_sn, None

    def effective(self, conv, channels_last: bool) -> torch.Tensor:
        if channels_last:
            raise NativeError("spectral normalisation (optim.spectral_norm) is fp32-path only: this convolution received a 16-bit channels-last tensor")
        if self.version != conv.weight._version:
            raise NativeError("spectral normalisation: the weight changed since W / sigma was last formed (an optimiser step, load_state_dict, init) — call "
                              "SpectralNorm.update() after the step, or refresh() after loading")
        return self.w_sn

    def __deepcopy__(self, memo):
        return None


def is_spectral(conv) -> bool:
    return conv.__dict__.get("_dcv_spectral") is not None


class SpectralNorm:
    """Spectral normalisation of nn.Conv2d / nn.Conv3d weights on the device: the convolutions compute with W / sigma(W), the Parameter stays W.

        sn = spectral_norm(models, guard=opt_idis.guard)      # marks the convolutions, registers weight_u / weight_v / weight_sigma, 15 power iterations
        loss.backward(); sn.project()                          # p.grad (the sum over every use of W / sigma): dL/d(W / sigma) -> dL/dW, once per optimiser step
        guard.measure(); opt.step() ...; sn.update()           # one power iteration and a new W / sigma per weight VERSION, right after the steps

    W is (cout, cin * kd * kh * kw): torch.nn.utils.spectral_norm's dim = 0, its formulas and its eps.  torch updates u, v at every forward; here they — and sigma
    — stay fixed between two optimiser steps, which is what makes one projection of the summed gradient valid and keeps the packed weights of W / sigma valid over
    the two or three uses of a discriminator per iteration.  A zero matrix gives W / sigma = 0 (torch: NaN).  With a ``guard`` the update applies — or skips on —
    the guard's last measurement, like the optimiser steps on it.  Nothing here reads a value on the host, runs a torch kernel or allocates in the steady state; the
    same bits in give the same bits out, so data-parallel replicas stay identical without a collective.  GPU only, fp32 only."""

    def __init__(self, modules, n_init: int = 15, eps: float = 1e-12, seed: int = 0, guard: Optional[GradGuard] = None):
        if not float(eps) > 0.0:
            raise ValueError(f"SpectralNorm: eps must be positive, got {eps!r}")
        if int(n_init) != n_init or int(n_init) < 0:
            raise ValueError(f"SpectralNorm: n_init must be a non-negative integer, got {n_init!r}")
        self.eps, self.guard = float(eps), guard
        self._dp: List["DataParallelAdam"] = []      # wrappers whose buckets project() reduces first (trainer.build_spectral_norm; a guard's are taken from it)
        self.convs: List[torch.nn.Module] = []
        seen = set()
        for m in modules:
            for sub in m.modules():
                if isinstance(sub, (torch.nn.ConvTranspose1d, torch.nn.ConvTranspose2d, torch.nn.ConvTranspose3d)):
                    raise NativeError("spectral_norm: ConvTranspose layers are not supported (their matrix is the other axis; no discriminator has one)")
                if isinstance(sub, (torch.nn.Conv2d, torch.nn.Conv3d)) and id(sub) not in seen:
                    seen.add(id(sub))
                    self.convs.append(sub)
        if not self.convs:
            raise ValueError("spectral_norm: no Conv2d / Conv3d to mark")
        for c in self.convs:      # every refusal before the first mark
            if is_spectral(c):
                raise NativeError("spectral_norm: a convolution is already marked")
            if c.weight.dtype != torch.float32 or not c.weight.is_contiguous():
                raise NativeError("spectral_norm: weights must be contiguous float32")
        gen = torch.Generator().manual_seed(int(seed))      # the same seed on every rank: replicas start from the same u, v
        for c in self.convs:
            w = c.weight
            rows, cols = w.shape[0], w[0].numel()
            u = torch.nn.functional.normalize(torch.randn(rows, generator=gen, dtype=torch.float64), dim=0, eps=self.eps).float()
            v = torch.nn.functional.normalize(torch.randn(cols, generator=gen, dtype=torch.float64), dim=0, eps=self.eps).float()
            c.register_buffer("weight_u", u.to(w.device))      # (host tensor -> device copies, once, before training: no kernel)
            c.register_buffer("weight_v", v.to(w.device))
            c.register_buffer("weight_sigma", torch.ones(1).to(w.device))
            c.__dict__["_dcv_spectral"] = _SpectralMark(torch.zeros(w.shape, dtype=torch.float32).to(w.device))
        self._tables = None
        self._ws: Optional[torch.Tensor] = None
        if self.convs[0].weight.is_cuda:      # host models can be marked (checkpoint layout, tests without a GPU); update() refuses them
            self.update(n_iter=int(n_init), _guarded=False)

    def remove(self):
        """Unmark: the convolutions compute with their raw weights again and lose the three buffers."""
        for c in self.convs:
            c.__dict__.pop("_dcv_spectral", None)
            for k in ("weight_u", "weight_v", "weight_sigma"):
                c._buffers.pop(k, None)
                c._non_persistent_buffers_set.discard(k)
        self.convs = []

    def _table(self) -> PointerTable:
        ts = [(c.weight, c.__dict__["_dcv_spectral"].w_sn, c.weight_u, c.weight_v, c.weight_sigma) for c in self.convs]
        self._tables = PointerTable.cached(self._tables, tuple(t.data_ptr() for row in ts for t in row), lambda: self._build_table(ts))
        return self._tables

    def _build_table(self, ts) -> dict:
        for i, row in enumerate(ts):
            for t in row:
                _require(t.data, f"SpectralNorm tensor of convolution {i}")
                if not t.is_contiguous():
                    raise NativeError("SpectralNorm: tensors must be contiguous")
            w, w_sn, u, v, sg = row
            if w_sn.shape != w.shape or u.numel() != w.shape[0] or v.numel() != w[0].numel() or sg.numel() != 1:
                raise NativeError(f"SpectralNorm: the buffers of convolution {i} do not fit its weight {tuple(w.shape)}")
        n = len(ts)
        w, w_sn, u, v, sigma = (c_array(col) for col in zip(*ts))
        rows, cols = c_array([row[0].shape[0] for row in ts], C.c_int32), c_array([row[0][0].numel() for row in ts], C.c_int32)
        need = lib().dcv_spectral_workspace_bytes(n, rows, cols)
        if need == 0:
            raise NativeError("dcv_spectral_workspace_bytes: " + lib().dcv_last_error().decode(errors="replace"))
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=ts[0][0].device)
        return dict(n=n, w=w, w_sn=w_sn, u=u, v=v, sigma=sigma, rows=rows, cols=cols, touched=[row[1] for row in ts])

    @torch.no_grad()
    def update(self, n_iter: int = 1, _guarded: bool = True):
        """`n_iter` power iterations from the stored u, v, then sigma and W / sigma, for every marked convolution; records each weight's version."""
        t = self._table()      # every refusal before the first launch
        state = ptr(self.guard._need_state()) if (self.guard is not None and _guarded) else None
        check(lib().dcv_spectral_update_multi(t.n, t.w, t.w_sn, t.u, t.v, t.sigma, t.rows, t.cols, int(n_iter), self.eps, state, ptr(self._ws), self._ws.numel(),
                                              stream_ptr()), "dcv_spectral_update_multi")
        # the kernels wrote through raw pointers: the packed-weight caches of W / sigma are keyed on its version counter (harmless after a skipped update)
        torch.autograd.graph.increment_version(t.touched)
        for c in self.convs:
            c.__dict__["_dcv_spectral"].version = c.weight._version

    def refresh(self):
        """sigma and W / sigma of the current weights and the stored u, v (no power iteration, never skipped): after load_state_dict."""
        self.update(n_iter=0, _guarded=False)

    @torch.no_grad()
    def project(self):
        """p.grad <- (G - <G, W / sigma> u v^T) / sigma for every marked weight that has a gradient: G is what the weight-gradient kernels summed over every use of
        W / sigma since zero_grad.  Once per optimiser step, before the guard measures."""
        for w in list(self._dp) + (list(self.guard._dp) if self.guard is not None else []):
            w.reduce_gradients()      # data parallel: never write a slice a collective is still reading, and project the SUM over the ranks (linear)
        t = self._table()
        idx, gs = [], []
        for i, c in enumerate(self.convs):
            g = c.weight.grad
            if g is None:
                continue
            _require(g, "SpectralNorm gradient")
            if not g.is_contiguous() or g.shape != c.weight.shape:
                raise NativeError("SpectralNorm: gradients must be contiguous and of the weight's shape")
            idx.append(i); gs.append(g.data_ptr())
        if not idx:
            return
        pick = lambda arr, ty=C.c_void_p: c_array([arr[i] for i in idx], ty)
        check(lib().dcv_spectral_project_multi(len(idx), c_array(gs), pick(t.w_sn), pick(t.u), pick(t.v), pick(t.sigma), pick(t.rows, C.c_int32),
                                               pick(t.cols, C.c_int32), self.eps, ptr(self._ws), self._ws.numel(), stream_ptr()), "dcv_spectral_project_multi")

    def state_dict(self):
        """u, v, sigma per marked convolution in marking order (they are also buffers of the modules, so a model checkpoint already carries them) and eps."""
        return {"eps": self.eps, "u": [c.weight_u.detach().cpu().clone() for c in self.convs], "v": [c.weight_v.detach().cpu().clone() for c in self.convs],
                "sigma": [c.weight_sigma.detach().cpu().clone() for c in self.convs]}

    @torch.no_grad()
    def load_state_dict(self, sd):
        """Loads u, v, sigma; W / sigma is stale afterwards — a marked convolution refuses to run until refresh()."""
        if not (len(sd["u"]) == len(sd["v"]) == len(sd["sigma"]) == len(self.convs)):
            raise ValueError(f"SpectralNorm.load_state_dict: {len(sd['u'])} layers in the checkpoint, {len(self.convs)} marked")
        self.eps = float(sd["eps"])
        for c, u, v, s in zip(self.convs, sd["u"], sd["v"], sd["sigma"]):
            c.weight_u.copy_(u); c.weight_v.copy_(v); c.weight_sigma.copy_(s)
            c.__dict__["_dcv_spectral"].version = None


def spectral_norm(models_or_modules, names=("idis", "vdis", "gdis"), n_init: int = 15, eps: float = 1e-12, seed: int = 0,
                  guard: Optional[GradGuard] = None) -> SpectralNorm:
    """Mark every Conv2d / Conv3d of the models `names` of a dict (or of a module / a sequence of modules) for spectral normalisation and return the handle that
    updates and projects them (SpectralNorm).  Raises on a ConvTranspose layer.  fp32 path only."""
    if isinstance(models_or_modules, dict):
        mods = [models_or_modules[n] for n in names]
    elif isinstance(models_or_modules, torch.nn.Module):
        mods = [models_or_modules]
    else:
        mods = list(models_or_modules)
    return SpectralNorm(mods, n_init=n_init, eps=eps, seed=seed, guard=guard)
