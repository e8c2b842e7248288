"""One G+D training iteration with the reference trainer's exact schedule.

Restates /root/reference/src/trainer.py:279-363 (the reference file itself cannot
ship: it imports evan / skvideo / colorlog / tensorboardX at module top, SURVEY
§0 D8) over objects with the reference's duck types — so it also drives the
reference's own classes, and a DCVGAN-style trainer drives ours.

Kept quirks: D-phase fakes are NOT detached (the dead generator backward runs),
``opt_ggen.step()`` is called twice, generators stay in whatever mode they were
left in until the first G phase, update gating by num_gen_update / num_dis_update.
Losses are returned as 0-d device tensors; ``sync_losses=True`` reproduces the
reference's four ``.cpu().item()`` host syncs per iteration.
"""
from __future__ import annotations

import collections
import os
from typing import Dict, Optional

import torch

from . import discriminator as D
from . import generator as G
from . import loss as Lm
from . import ops, optim, util
from .configs import StepConfig

MODEL_NAMES = ("ggen", "cgen", "idis", "vdis", "gdis")


def build_models(cfg: StepConfig, device=None, sync_bn: bool = False) -> Dict[str, torch.nn.Module]:
    """train.py:117-165: positional constructor wiring + init_weights.
    `sync_bn` (data parallel, fp32 path; default off): every BatchNorm of the five models takes its statistics over the batch of all ranks
    (optim.sync_batchnorm; a collective call, every rank makes it).  optim.sync_bn_group_of(models) returns the handle afterwards."""
    w = cfg.width
    ggen = G.GeometricVideoGenerator(cfg.dim_z_content, cfg.dim_z_motion, cfg.channel, cfg.geometric_info, w["ggen"], cfg.video_length)
    cgen = G.ColorVideoGenerator(ggen.channel, cfg.dim_z_color, cfg.geometric_info, w["cgen"], cfg.video_length)
    idis = D.ImageDiscriminator(ggen.channel, cgen.channel, cfg.use_noise["idis"], cfg.noise_sigma["idis"], w["idis"])
    vdis = D.VideoDiscriminator(ggen.channel, cgen.channel, cfg.use_noise["vdis"], cfg.noise_sigma["vdis"], w["vdis"])
    gdis = D.GradientDiscriminator(ggen.channel, cgen.channel, cfg.use_noise["gdis"], cfg.noise_sigma["gdis"], w["gdis"])
    models = dict(ggen=ggen, cgen=cgen, idis=idis, vdis=vdis, gdis=gdis)
    for m in models.values():
        m.apply(util.init_weights)
        m.to(device if device is not None else util.current_device())
    if sync_bn:
        optim.sync_batchnorm(models)
    return models


def build_loss(cfg: StepConfig):
    return Lm.AdversarialLoss() if cfg.loss == "adversarial-loss" else Lm.HingeLoss()


def build_optimizers(cfg: StepConfig, models, data_parallel: bool = False, overlap: Optional[bool] = None, guard: Optional[dict] = None):
    """train.py:169-176.  Data parallel: the optimisers stepped after the same backward share one gradient
    bucket — D phase (trainer.py:319-322) and G phase (trainer.py:356-359) — so an iteration has two collectives.
    `overlap` (default: the environment's DCV_DP_OVERLAP, else off): per-model chunks whose collectives start from the hook of the chunk's last gradient, on a
    communication stream, while the rest of the backward runs (optim.GradBucket(overlap=True)); off by default until an N > 1 run has measured it.
    `guard`: keyword arguments of optim.GradGuard, e.g. dict(max_norm=10.0) — one guard per phase with the buckets' grouping (D: idis + vdis + gdis, G: ggen + cgen),
    reachable as `opts[name].guard`; StepRunner then measures after each backward and every step applies the guard's decision.  None (default): no guard."""
    opts = {}
    if overlap is None:
        overlap = os.environ.get("DCV_DP_OVERLAP") is not None
    buckets = {"D": optim.GradBucket(overlap=overlap), "G": optim.GradBucket(overlap=overlap)} if data_parallel else None
    guards = {"D": optim.GradGuard(**guard), "G": optim.GradGuard(**guard)} if guard is not None else {"D": None, "G": None}
    for name in MODEL_NAMES:
        phase = "D" if name.endswith("dis") else "G"
        o = optim.Adam(models[name].parameters(), lr=cfg.lr[name], betas=(0.5, 0.999), weight_decay=cfg.decay[name], guard=guards[phase])
        opts[name] = optim.DataParallelAdam(o, buckets[phase]) if data_parallel else o
    return opts


def build_ema(cfg: StepConfig, models, optimizers, decay: float = 0.999, warmup: bool = True) -> "optim.ModelEma":
    """The sampling twins of the two generators (optim.ModelEma), wired to the G phase's guard when build_optimizers made one: the three G steps and the EMA
    update then share one measurement and are all applied or all skipped.  Hand it to StepRunner(..., ema=...)."""
    return optim.ModelEma(models, names=("ggen", "cgen"), decay=decay, warmup=warmup, guard=getattr(optimizers["ggen"], "guard", None))


def build_spectral_norm(cfg: StepConfig, models, optimizers, names=("idis", "vdis", "gdis"), n_init: int = 15, eps: float = 1e-12,
                        seed: int = 0) -> "optim.SpectralNorm":
    """Spectral normalisation of the discriminators' convolutions (optim.spectral_norm), wired to the D phase's guard when build_optimizers made one — the three D
    steps and the power iteration then share one measurement and are all applied or all skipped — and to the data-parallel wrappers, whose bucket the projection
    reduces first.  Hand it to StepRunner(..., spectral=...).  fp32 path only."""
    sn = optim.spectral_norm(models, names=names, n_init=n_init, eps=eps, seed=seed, guard=getattr(optimizers[names[0]], "guard", None))
    sn._dp = [optimizers[n] for n in names if hasattr(optimizers[n], "reduce_gradients")]
    return sn


def build_augment(cfg: StepConfig, models, optimizers, **kw) -> "augment.ClipAugment":
    """Adaptive clip augmentation in front of the three discriminators (augment.ClipAugment) on the models' device; keyword arguments are the
    constructor's (p, adaptive, target, interval, p_max, adjust_clips, ops, seed, ...).  Hand it to StepRunner(..., augment=...).  fp32 path only.  Under data
    parallelism every rank makes this call (it creates a process group); the per-rank batch is cfg.batchsize, so `batch` defaults to batchsize x world."""
    from . import augment
    import torch.distributed as dist
    world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
    kw.setdefault("batch", cfg.batchsize * world)
    return augment.ClipAugment(cfg, next(models["idis"].parameters()).device, **kw)


def build_lecam(cfg: StepConfig, models, optimizers, **kw) -> "lecam.LeCam":
    """LeCam regularisation of the three discriminators (lecam.LeCam) on the models' device; keyword arguments are the constructor's (weight — required —
    decay, start, one_sided).  Hand it to StepRunner(..., lecam=...).  fp32 path only.  Under data parallelism every rank makes this call (it creates a process
    group)."""
    from . import lecam
    kw.setdefault("device", next(models["idis"].parameters()).device)
    return lecam.LeCam(3, **kw)


def build_clip_sampler(cfg: StepConfig, store, **kw) -> "clipstore.ClipSampler":
    """The real batches of the run, made on the device from a clipstore.ClipStore instead of a DataLoader (train.py:101-109, trainer.py:271): per-rank
    batches of cfg.batchsize; keyword arguments are the sampler's (seed, rank, world — by default torch.initial_seed() and torch.distributed's rank and world).  Feed
    ``runner.step(batch["color"], batch[cfg.geometric_info], t_rand)``.  No collective call: every rank computes its own slice of the epoch."""
    from . import clipstore
    if store.geometric_info != cfg.geometric_info or store.video_length != cfg.video_length:
        raise ValueError(f"build_clip_sampler: the store holds {store.geometric_info} clips of {store.video_length} frames, the config asks for "
                         f"{cfg.geometric_info} clips of {cfg.video_length}")
    return clipstore.ClipSampler(store, kw.pop("batchsize", cfg.batchsize), **kw)


def build_evaluator(cfg: StepConfig, models, extractor, ema=None, **kw) -> "evaluation.Evaluator":
    """On-device evaluation in place of Trainer.evaluate (trainer.py:171-224): an evaluation.Evaluator bound to the two generators — with `ema`
    (optim.ModelEma, build_ema) to their EMA twins, the weights a GAN is evaluated from — so that ``ev.evaluate(num_samples=..., batchsize=...)`` needs no models.
    `extractor(xc) -> (features, logits or None)` is the caller's feature network; keyword arguments are the Evaluator's (metrics, max_features, kid_subsets,
    kid_subset_size, seed, real_moments, prd_clusters, prd_runs, prd_iters, pr_k, dc_k): ``metrics=("fid", "pr", "dc")`` adds improved precision / recall
    (pr_k = 3 neighbours) and density / coverage (dc_k = 5) over the stored features, ``"prcurve"`` the reference's "prd" (DESIGN §18).  Feed the real statistics once with ``ev.observe_real(batch["color"])``."""
    from . import evaluation
    ev = evaluation.Evaluator(extractor, **kw)
    ev.ggen, ev.cgen = (ema.module("ggen"), ema.module("cgen")) if ema is not None else (models["ggen"], models["cgen"])
    return ev


MONITOR_GROUPS = tuple(f"{d}_{k}" for d in ("idis", "vdis", "gdis") for k in ("real", "fake_d", "fake_g"))


def build_monitor(cfg: StepConfig, models, optimizers, interval: int = 100, lecam=None, **kw) -> "monitor.RunMonitor":
    """The training log kept on the device (monitor.RunMonitor) in place of the reference's logger.update(..., loss.cpu().item()) / logger.log()
    (trainer.py:326-328,363; logger.py:144-148,280-283).  The slots are what the run's ``step()`` returns, in this fixed order: loss_idis, loss_vdis, loss_gdis,
    loss_gen; lecam_idis, lecam_vdis, lecam_gdis if `lecam` is given; grad_norm_dis, skipped_dis, grad_norm_gen, skipped_gen if the optimisers are guarded.  The
    nine logit groups are {idis, vdis, gdis} x {real, fake_d (the D phase's fakes), fake_g (the G phase's)}.  Hand it to StepRunner(..., monitor=...), which observes
    once per iteration and rolls every `interval` iterations; keyword arguments are the constructor's (ring).  Data parallel: each rank monitors its own batch; no
    collective is added."""
    from . import monitor
    slots = ["loss_idis", "loss_vdis", "loss_gdis", "loss_gen"]
    if lecam is not None:
        slots += ["lecam_idis", "lecam_vdis", "lecam_gdis"]
    if getattr(optimizers["idis"], "guard", None) is not None:
        slots += ["grad_norm_dis", "skipped_dis"]
    if getattr(optimizers["ggen"], "guard", None) is not None:
        slots += ["grad_norm_gen", "skipped_gen"]
    kw.setdefault("device", next(models["idis"].parameters()).device)
    return monitor.RunMonitor(slots, MONITOR_GROUPS, interval=interval, **kw)


def build_run_state(cfg: StepConfig, models, optimizers, runner=None, ema=None, spectral=None, augment=None, lecam=None, sampler=None, rngs=(), extra=None,
                    slots: int = 2, monitor=None) -> "runstate.RunState":
    """Everything the run has become, as one object (runstate.RunState): ``capture()`` packs the models, Adam moments, guard, EMA twins, augmentation
    and LeCam state into a device arena on the current stream and copies the host scalars; the snapshot restores in memory (rollback) or through one file (resume in
    fresh objects, bit for bit); ``fingerprint()`` digests the live state without a copy.  Hand over the same objects StepRunner got; ``rngs`` are random streams
    of the caller's own, ``extra`` a dict of the caller's plain values (the generator behind ``t_rand`` belongs there).  The iteration itself is untouched.
    `monitor` (build_monitor): its live window becomes part of the state."""
    from . import runstate
    return runstate.RunState(models, optimizers, runner=runner, ema=ema, spectral=spectral, augment=augment, lecam=lecam, sampler=sampler, rngs=rngs, extra=extra,
                             slots=slots, monitor=monitor)


class StepRunner:
    """`elide_dead_backward=True` builds the D-phase fakes without a tape (they are detached): the
    reference backpropagates `loss_dis` through cgen/ggen too (trainer.py:304-319, fakes not detached)
    and then throws those gradients away with `zero_grad()` at :340-341, so parameters, buffers and
    losses are identical either way; only ~23 % of the step's FLOPs disappear (BASELINE.md §4,
    "minimal" column).  Default False = the reference's as-written schedule."""

    def __init__(self, cfg: StepConfig, models, optimizers, loss, sync_losses: bool = False, elide_dead_backward: bool = False,
                 side_streams: Optional[bool] = None, ema: Optional["optim.ModelEma"] = None, spectral: Optional["optim.SpectralNorm"] = None,
                 augment: Optional["augment.ClipAugment"] = None, lecam: Optional["lecam.LeCam"] = None, monitor: Optional["monitor.RunMonitor"] = None):
        self.cfg, self.models, self.opt, self.loss = cfg, models, optimizers, loss
        # monitor.RunMonitor (build_monitor): at the end of step() the iteration's scalars and the nine logits tensors are folded into its device window (one launch,
        # on the main stream after the lanes have joined), and every monitor.interval iterations the window is published (one more); it only reads: parameters,
        # buffers, losses and random draws are those of the run without it; None leaves the iteration as it is
        if monitor is not None and sync_losses:
            raise ValueError("StepRunner: monitor and sync_losses=True exclude one another: with sync_losses the iteration's values are Python floats read on the host "
                             "(the reference's way), and the monitor takes device scalars and does not upload")
        self.monitor = monitor
        # lecam.LeCam (build_lecam): the D phase forms its three losses through it — loss_idis / loss_vdis / loss_gdis of step()'s result then INCLUDE their regulariser
        # term, which the result also carries alone as lecam_idis / lecam_vdis / lecam_gdis — and the anchors move every iteration, also one whose D update is gated
        # off or skipped by the guard (they are statistics of the outputs, not of the weights); the G phase is untouched; None leaves the iteration as it is
        self.lecam = lecam
        # augment.ClipAugment (build_augment): the real pair and each phase's fakes pass through it on their way to the discriminators (cgen still reads the
        # un-augmented geometry clip); None leaves the iteration as it is
        self.augment = augment
        # optim.SpectralNorm (build_spectral_norm): in the D phase the summed gradients are projected before the guard measures, and W / sigma is renewed right after
        # the three steps, on the optimiser's stream (the lanes see it ordered as they see the new weights); None leaves the iteration as it is
        self.spectral = spectral
        self.ema = ema      # optim.ModelEma (build_ema): updated once per iteration whose G phase stepped, after its three steps; None leaves the iteration as it is
        self.iteration = 0
        self.sync_losses = sync_losses
        self.elide_dead_backward = elide_dead_backward
        if side_streams is None:
            side_streams = os.environ.get("DCV_NO_SIDE_STREAMS") is None
        self._lanes = None
        dev = next(models["idis"].parameters()).device
        if side_streams and dev.type == "cuda":
            self._lanes = [torch.cuda.Stream(dev) for _ in range(3)]
        if cfg.start_in_eval:  # trainer.py:266-267: log_samples/evaluate leave the generators in eval()
            models["ggen"].eval(); models["cgen"].eval()
        # diagnostics (tools/phases.py): HIP events on the main stream at the phase boundaries of an iteration; None = off (no event is ever recorded)
        self.phase_marks = None
        self._ones = {}
        # How many iterations the host may enqueue ahead of the GPU.  The reference's loop reads the losses on the host every iteration (trainer.py:326-328,363) and is
        # never ahead; a caller that does not (bench.py, sync_losses=False) enqueues an iteration in about a third of the time the GPU takes to run it, and every tensor
        # that crossed streams is only returned to the allocator when the GPU reaches its last use — without a bound the memory in flight grows with the lead (soak at
        # B = 70: 37 GB after 5 iterations, 146 GB allocated / 191 GB reserved after 150).  Two iterations keep the GPU's queues full and the memory flat.
        self.max_ahead = max(1, int(os.environ.get("DCV_MAX_ITERATIONS_AHEAD", "2")))
        self._inflight = collections.deque()
        # optim.GradGuard of each phase (build_optimizers(guard=...)); None — also for optimisers that know no guard — leaves the iteration as it is without one
        self._guard_dis = getattr(optimizers["idis"], "guard", None)
        self._guard_gen = getattr(optimizers["ggen"], "guard", None)

    def _mark(self, name):
        if self.phase_marks is not None:
            e = torch.cuda.Event(enable_timing=True)
            e.record(torch.cuda.current_stream())
            self.phase_marks.append((name, e))

    # The three discriminators are independent of one another (trainer.py:299-309, 347-349): each runs on its own HIP stream, so
    # their small layers (70-frame image discriminator, the 1-channel heads, BN reductions) and the tail rounds of the large ones
    # fill one another's idle CUs.  Autograd replays every tape entry on the stream of its forward and orders producer/consumer
    # streams itself, and joins the leaf streams with the caller's at the end of backward(); the host order of all calls — hence
    # every random draw and every result bit — is that of the single-stream schedule.
    def _on_lanes(self, dis, call, join: bool = True):
        if self._lanes is None:
            return tuple(call(d) for d in dis)
        main = torch.cuda.current_stream()
        outs = []
        for lane, d in zip(self._lanes, dis):
            lane.wait_stream(main)          # inputs (and the optimiser's updates) were produced on the main stream
            with torch.cuda.stream(lane):
                outs.append(call(d))
        if join:
            self._adopt(outs)
        return tuple(outs)

    def _adopt(self, outs):
        if self._lanes is None:
            return
        main = torch.cuda.current_stream()
        for lane, y in zip(self._lanes, outs):
            main.wait_stream(lane)
            y.record_stream(main)           # allocated on the lane, read by the loss kernels on the main stream

    # The fake clips are read by three discriminators — the image discriminator takes frame t_rand — and the geometry clip by the colour generator too
    # (trainer.py:303-309, 344-349).  ops.fan_out hands every consumer a view and forms the clip's ONE gradient with the library's kernels; left to autograd the fan-in
    # is a torch add per extra consumer plus the zero-fill + copy of each slice's backward (18 + ~25 torch launches per iteration in round 5's traces).
    def _colour(self, cgen, xg_fake, t_rand):
        """-> ((frame, for vdis, for gdis) of the geometry clip, the same of the colour clip cgen makes of it)"""
        if self.augment is not None:
            return self._colour_augmented(cgen, xg_fake, t_rand)
        if not (xg_fake.is_cuda and xg_fake.requires_grad):
            xc = cgen.forward_videos(xg_fake)
            return (xg_fake[:, :, t_rand], xg_fake, xg_fake), (xc[:, :, t_rand], xc, xc)
        g_i, g_c, g_v, g_g = ops.fan_out(xg_fake, t_rand, 3)
        c_i, c_v, c_g = ops.fan_out(cgen.forward_videos(g_c), t_rand, 2)
        return (g_i, g_v, g_g), (c_i, c_v, c_g)

    def _colour_augmented(self, cgen, xg_fake, t_rand):
        """_colour with the augmentation between the generators and the discriminators: cgen reads the clip as ggen made it and the augmented pair (one draw) is what
        fans out to the three discriminators.  The colour clip's fan-in stays ops.fan_out; the geometry clip's four readers meet in augment._AugFan."""
        if not (xg_fake.is_cuda and xg_fake.requires_grad):
            yg, yc = self.augment(xg_fake, cgen.forward_videos(xg_fake))
            return (yg[:, :, t_rand], yg, yg), (yc[:, :, t_rand], yc, yc)
        aug = self.augment
        table = aug.draw(xg_fake.shape[0], xg_fake.shape[3], xg_fake.shape[4])
        g_c, g_i, g_v, g_g = aug.fan_geometry(xg_fake, t_rand, table)      # the geometry clip's ONE gradient: one launch, in ops.fan_out's order of additions
        yc = aug.colour(cgen.forward_videos(g_c), table)
        return (g_i, g_v, g_g), ops.fan_out(yc, t_rand, 2)

    def _fakes_through(self, dis, idis, xg, xc, t_rand):
        which = {id(d): k for k, d in enumerate(dis)}
        return self._on_lanes(dis, lambda d: d(xg[which[id(d)]], xc[which[id(d)]]))

    def _root(self, loss):
        """d loss / d loss = 1 as a cached device scalar (backward() without an argument fills a fresh ones_like with a torch kernel)."""
        one = self._ones.get(loss.device)
        if one is None:
            one = self._ones[loss.device] = torch.ones((), dtype=loss.dtype, device=loss.device)
        return one

    def _guard_report(self, out, guard, phase):
        """grad_norm_<phase> / skipped_<phase> of the guard's last measurement: a snapshot of its state (one dcv_axpby launch), since the state itself moves on with the
        next measurement while the host runs ahead."""
        snap = ops._axpby(guard.state.view(1, -1), 1.0, None, 0.0, torch.empty((1, guard.state.numel()), dtype=torch.float32, device=guard.state.device))[0]
        norm, skipped = snap[guard.FIELDS.index("grad_norm")], snap[guard.FIELDS.index("skipped")]
        out["grad_norm_" + phase] = norm.cpu().item() if self.sync_losses else norm
        out["skipped_" + phase] = skipped.cpu().item() if self.sync_losses else skipped

    def step(self, xc_real: torch.Tensor, xg_real: torch.Tensor, t_rand: int):
        c, m, o = self.cfg, self.models, self.opt
        guard_dis, guard_gen = self._guard_dis, self._guard_gen
        ggen, cgen, idis, vdis, gdis = (m[k] for k in MODEL_NAMES)
        self.iteration += 1
        if xc_real.is_cuda:
            while len(self._inflight) >= self.max_ahead:
                self._inflight.popleft().synchronize()      # the host waits for iteration i - max_ahead to END: no kernel of the current queue is delayed
        # ---- discriminator phase (trainer.py:285-328) ----
        for d in (idis, vdis, gdis):
            d.train()
        for d in (idis, vdis, gdis):
            d.zero_grad()
        dis = (idis, vdis, gdis)
        self._mark("start")
        if self.augment is not None:
            xg_real, xc_real = self.augment(xg_real, xc_real)      # once per iteration, before the D lanes start
        y_real = self._on_lanes(dis, lambda d: d(xg_real[:, :, t_rand], xc_real[:, :, t_rand]) if d is idis else d(xg_real, xc_real), join=False)
        with torch.set_grad_enabled(not self.elide_dead_backward):
            xg_fake = ggen.sample_videos(c.batchsize)     # on the main stream, beside the discriminators' real-batch passes
            xg_fake, xc_fake = self._colour(cgen, xg_fake, t_rand)
        self._mark("D: generators forward (beside D on the real batch)")
        y_fake = self._fakes_through(dis, idis, xg_fake, xc_fake, t_rand)
        self._adopt(y_real)
        if self.augment is not None:
            for y in y_real:
                self.augment.observe(y)      # r = E[sign(D(real))]: integer sums on the device (adaptive mode only)
        self._mark("D: discriminators forward on the fakes")
        if self.lecam is not None:
            loss_idis, loss_vdis, loss_gdis = self.lecam.compute_dis_losses(self.loss, y_real, y_fake)      # the GAN terms + the regulariser: 2 more launches
        else:
            loss_idis = self.loss.compute_dis_loss(y_real[0], y_fake[0])
            loss_vdis = self.loss.compute_dis_loss(y_real[1], y_fake[1])
            loss_gdis = self.loss.compute_dis_loss(y_real[2], y_fake[2])
        loss_dis = ops.sum_scalars(loss_idis, loss_vdis, loss_gdis) if loss_idis.is_cuda else loss_idis + loss_vdis + loss_gdis      # trainer.py:315
        d_steps = self.iteration % c.num_gen_update == 0      # the D phase's gate, decided once (the monitor reads it again below)
        if d_steps:
            loss_dis.backward(guard_dis.root(loss_dis) if guard_dis is not None else self._root(loss_dis))
            self._mark("D: backward (D lanes, then the generators' dead backward)")
            if self.spectral is not None:
                self.spectral.project()      # dL/d(W / sigma), summed over the real and the fake batch -> dL/dW (the G phase's gradients into D are never stepped)
            if guard_dis is not None:
                guard_dis.measure()
            o["idis"].step(); o["vdis"].step(); o["gdis"].step()
            if self.spectral is not None:
                self.spectral.update()       # one power iteration per weight version
            self._mark("D: Adam")
        else:
            loss_dis.detach_()
        if self.sync_losses:   # trainer.py:326-328 — on the loss objects themselves, as the reference reads them (they carry a host mirror: loss.HostMirroredLoss)
            out = {"loss_idis": loss_idis.cpu().item(), "loss_vdis": loss_vdis.cpu().item(), "loss_gdis": loss_gdis.cpu().item()}
        else:
            out = {"loss_idis": loss_idis.detach(), "loss_vdis": loss_vdis.detach(), "loss_gdis": loss_gdis.detach()}
        if self.lecam is not None:
            reg = self.lecam.reg.cpu().tolist() if self.sync_losses else self.lecam.reg      # (this iteration's own tensor: the next one writes another)
            out["lecam_idis"], out["lecam_vdis"], out["lecam_gdis"] = reg[0], reg[1], reg[2]
        if guard_dis is not None:
            self._guard_report(out, guard_dis, "dis")
        if self.augment is not None:
            self.augment.end_of_iteration(self.iteration)      # every `interval` iterations: p follows r (one thread; after an all-reduce of the sums under data parallelism)
        if self.monitor is not None:
            seen = {f"{n}_real": y.detach() for n, y in zip(("idis", "vdis", "gdis"), y_real)}
            seen.update({f"{n}_fake_d": y.detach() for n, y in zip(("idis", "vdis", "gdis"), y_fake)})
        del y_real, y_fake, xg_fake, xc_fake, loss_dis
        # ---- generator phase (trainer.py:338-363) ----
        ggen.train(); cgen.train()
        ggen.zero_grad(); cgen.zero_grad()
        xg_fake = ggen.sample_videos(c.batchsize)
        xg_fake, xc_fake = self._colour(cgen, xg_fake, t_rand)
        self._mark("G: generators forward")
        y_fake = self._fakes_through(dis, idis, xg_fake, xc_fake, t_rand)
        loss_gen = self.loss.compute_gen_loss(*y_fake)
        self._mark("G: discriminators forward on the fakes")
        g_steps = self.iteration % c.num_dis_update == 0      # the G phase's gate
        if g_steps:
            loss_gen.backward(guard_gen.root(loss_gen) if guard_gen is not None else self._root(loss_gen))
            self._mark("G: backward (D lanes, then the generators)")
            if guard_gen is not None:
                guard_gen.measure()
            o["ggen"].step(); o["cgen"].step(); o["ggen"].step()  # ggen twice — trainer.py:357-359
            if self.ema is not None:
                self.ema.update()      # once per iteration, not per step: both generators get the same averaging horizon
            self._mark("G: Adam")
        else:
            loss_gen.detach_()
        out["loss_gen"] = loss_gen.cpu().item() if self.sync_losses else loss_gen.detach()     # trainer.py:363
        if guard_gen is not None:
            self._guard_report(out, guard_gen, "gen")
        if self.monitor is not None:
            seen.update({f"{n}_fake_g": y.detach() for n, y in zip(("idis", "vdis", "gdis"), y_fake)})
            gated = ([] if d_steps else ["grad_norm_dis", "skipped_dis"]) + ([] if g_steps else ["grad_norm_gen", "skipped_gen"])
            # a gated phase measured nothing: its guard fields still hold the measurement before, and their slots are not observed
            self.monitor.observe({k: v for k, v in out.items() if k not in gated}, seen)
            if self.iteration % self.monitor.interval == 0:
                self.monitor.roll(self.iteration)
            del seen
        if xc_real.is_cuda:
            e = torch.cuda.Event()
            e.record(torch.cuda.current_stream())      # (the lanes and the companion stream have joined the main stream by now)
            self._inflight.append(e)
        return out
