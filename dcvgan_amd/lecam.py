"""LeCam regularisation of the discriminators, anchors kept on the device.

Tseng et al., "Regularizing GANs under limited data" (CVPR 2021): keep an exponential moving average of each discriminator's mean logit on the real and on the fake
batch — the anchors aR, aF — and add ``weight * (mean(relu(D(real) - aF)^2) + mean(relu(aR - D(fake))^2))`` to its loss.  It acts on the logits only, so it needs
neither a second-order backward nor anything of BatchNorm; it is what adaptive augmentation (augment.ClipAugment) is normally paired with on small datasets.

The public implementations read the batch means on the host every iteration.  Here the anchors, the warm-up switch, the value and the gradient live in device memory:
``dcv_lecam_sums`` forms the batch sums (all-reduced under data parallelism), ``dcv_lecam_apply`` folds the regulariser into the loss values and stored gradients
the ``dcv_gan_loss`` launches left, then moves the anchors.  Two launches per iteration, no torch kernel, no host read.  fp32 logits only.
"""
from __future__ import annotations

import ctypes as C
import struct
from typing import Sequence

import torch
from torch.autograd import Function

from . import loss as Lm
from . import native as N
from . import ops
from .native import NativeError, c_array, check, lib, ptr, stream_ptr

STATE_WORDS = 8                                        # anchor_real (fp32 bits), anchor_fake (fp32 bits), updates, active, 4 reserved
ANCHOR_REAL, ANCHOR_FAKE, UPDATES, ACTIVE = range(4)   # include/dcvgan_hip.h: DCV_LECAM_*
MAX_DIS, MAX_N = 8, 1 << 24                            # the kernels' limits
NAMES = ("idis", "vdis", "gdis")


def dis_kinds(loss) -> tuple:
    """The (real, fake) dcv_gan_loss kinds of `loss.compute_dis_loss`."""
    if isinstance(loss, Lm.AdversarialLoss):
        return ops.KIND_BCE_ONES, ops.KIND_BCE_ZEROS
    if isinstance(loss, Lm.HingeLoss):
        return ops.KIND_HINGE_REAL, ops.KIND_HINGE_FAKE
    raise NativeError(f"LeCam: no dcv_gan_loss kinds are known for a {type(loss).__name__} (loss.AdversarialLoss and loss.HingeLoss are)")


def _require_logits(t, what: str):
    if not isinstance(t, torch.Tensor):
        raise NativeError(f"{what}: expected a tensor, got {type(t).__name__}")
    N._require(t, what)        # a HIP device tensor, float32 (a 16-bit tensor is refused), on the current device
    if not 1 <= t.numel() <= MAX_N:
        raise NativeError(f"{what}: 1 to 2^24 logits, got {t.numel()}")


class _DisLosses(Function):
    """(y_real_0, y_fake_0, y_real_1, y_fake_1, ...) -> one 0-d loss per discriminator: the two dcv_gan_loss terms of each (value + stored gradient), then the
    regulariser folded into those same values and stored gradients.  Backward: each stored gradient times its loss's upstream 0-d cotangent (dcv_scale_dev), as
    ops._GanLoss does it — every logits tensor has this one consumer, so autograd adds nothing."""

    @staticmethod
    def forward(ctx, lc, kinds, *ys):
        n = len(ys) // 2
        for i, y in enumerate(ys):
            _require_logits(y, "LeCam: %s logits of discriminator %d" % ("fake" if i % 2 else "real", i // 2))
        ycs = [y.contiguous() for y in ys]      # (a discriminator's output is contiguous: no launch)
        dev = ycs[0].device
        outs = [ops._empty((), dev) for _ in range(n)]
        dys = [ops._empty(y.shape, dev) for y in ycs]
        L, s = lib(), stream_ptr()
        for i, y in enumerate(ycs):
            check(L.dcv_gan_loss(ptr(y), y.numel(), int(kinds[i % 2]), ptr(outs[i // 2]), i % 2, ptr(dys[i]), s), "dcv_gan_loss")
        lc._fold(ycs[0::2], ycs[1::2], outs, dys[0::2], dys[1::2])
        ctx.save_for_backward(*dys)
        ctx.shapes = [tuple(y.shape) for y in ys]
        ctx.set_materialize_grads(False)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *gs):
        outs = []
        for i, (dy, shape, need) in enumerate(zip(ctx.saved_tensors, ctx.shapes, ctx.needs_input_grad[2:])):
            g = gs[i // 2]
            if not need or g is None:
                outs.append(None)
                continue
            if not (g.is_cuda and g.dtype == torch.float32):
                raise NativeError("LeCam backward: the upstream cotangent must be an fp32 device tensor")
            dx = ops._empty(dy.shape, dy.device)
            check(lib().dcv_scale_dev(ptr(dy), dy.numel(), ptr(g.reshape(())), ptr(dx), stream_ptr()), "dcv_scale_dev")
            outs.append(dx.view(shape))
        return (None, None) + tuple(outs)


class LeCam:
    """``lc = LeCam(n_dis=3, weight=..., device=...)``; ``loss_idis, loss_vdis, loss_gdis = lc.compute_dis_losses(loss, y_reals, y_fakes)`` in place of the three
    ``loss.compute_dis_loss(y_real, y_fake)`` calls.  Each returned loss is its GAN loss plus, once the regulariser is active,
    ``weight * (mean(relu(y_real - aF)^2) + mean(relu(aR - y_fake)^2))`` (``one_sided=False``: without the relu, the paper's form).

    ``weight`` has no default: the paper's values span 1e-7 to 0.3 with the loss and the dataset.  ``decay`` (0.99) and ``start`` (1000 anchor updates before the
    regulariser is added; at least 1, since the first update only initialises the anchors) are this project's choice, not measured optima.

    The anchors a call uses are those of the iterations BEFORE it (constants of the call: no gradient flows through them); the first update sets them to the batch
    means; a batch whose mean is not finite leaves them alone.  They move with every call, whether or not the discriminators are stepped afterwards.

    ``lc.reg``: a (n_dis,) device tensor, the regulariser's value in each loss of the last call (0 while inactive); a fresh tensor per call, so a caller may keep it.
    Data parallel: with torch.distributed initialised and more than one rank, the batch sums are all-reduced (SUM, n_dis x 4 doubles) over a process group of this
    object's own between the two launches, so every rank holds the anchors of one process that sees the concatenated logits.  Constructing it is then a
    collective call."""

    def __init__(self, n_dis: int = 3, *, weight: float, decay: float = 0.99, start: int = 1000, one_sided: bool = True, device=None):
        if not 1 <= int(n_dis) <= MAX_DIS:
            raise ValueError(f"LeCam: 1 <= n_dis <= {MAX_DIS}, got {n_dis!r}")
        if not (float(weight) >= 0.0 and float(weight) != float("inf")) or not 0.0 <= float(decay) <= 1.0 or int(start) < 0:
            raise ValueError(f"LeCam: weight finite and >= 0, decay in [0, 1], start >= 0; got {weight!r}, {decay!r}, {start!r}")
        from . import util
        self.n_dis, self.weight, self.decay, self.start, self.one_sided = int(n_dis), float(weight), float(decay), int(start), bool(one_sided)
        self.device = torch.device(device if device is not None else util.current_device())
        # the state blocks, zeroed: host tensors copied to the device once (no kernel)
        self.state = torch.zeros(self.n_dis * STATE_WORDS, dtype=torch.int32).to(self.device)
        self.sums = torch.zeros((self.n_dis, 4), dtype=torch.float64).to(self.device)
        self.reg = torch.zeros(self.n_dis, dtype=torch.float32).to(self.device)
        self.pg, self.world = None, 1
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            self.pg, self.world = dist.new_group(), dist.get_world_size()
        self.calls = 0      # counters for tests / tools
        self.collectives = 0

    def _fold(self, y_reals, y_fakes, losses, dy_reals, dy_fakes):
        """dcv_lecam_sums, the collective, dcv_lecam_apply on contiguous fp32 device tensors: the regulariser goes into `losses` and `dy_*` in place."""
        n = self.n_dis
        if self.state.device.type != "cuda":
            raise NativeError(f"LeCam: the state is on {self.state.device} — the regulariser runs on the GPU only (there is no CPU fallback)")
        if not (len(y_reals) == len(y_fakes) == len(losses) == len(dy_reals) == len(dy_fakes) == n):
            raise NativeError(f"LeCam: built for {n} discriminators, got {len(y_reals)} real and {len(y_fakes)} fake logit tensors")
        for k in range(n):
            for t, like, what in ((y_reals[k], None, "real logits"), (y_fakes[k], None, "fake logits"), (dy_reals[k], y_reals[k], "real gradient"),
                                  (dy_fakes[k], y_fakes[k], "fake gradient"), (losses[k], None, "loss")):
                _require_logits(t, f"LeCam: {what} of discriminator {k}")
                if not t.is_contiguous() or (like is not None and t.numel() != like.numel()) or (what == "loss" and t.numel() != 1):
                    raise NativeError(f"LeCam: {what} of discriminator {k}: expected a contiguous tensor of matching size, got {tuple(t.shape)}")
        yr, yf = c_array(y_reals), c_array(y_fakes)
        nr, nf = c_array([t.numel() for t in y_reals], C.c_int64), c_array([t.numel() for t in y_fakes], C.c_int64)
        reg = torch.empty(n, dtype=torch.float32, device=self.state.device)
        L, s = lib(), stream_ptr()
        check(L.dcv_lecam_sums(n, yr, yf, nr, nf, ptr(self.sums), s), "dcv_lecam_sums")
        if self.world > 1:
            import torch.distributed as dist
            dist.all_reduce(self.sums, op=dist.ReduceOp.SUM, group=self.pg)
            self.collectives += 1
        check(L.dcv_lecam_apply(n, yr, yf, nr, nf, ptr(self.sums), ptr(self.state), self.decay, self.start, self.weight, int(self.one_sided),
                                c_array(losses), c_array(dy_reals), c_array(dy_fakes), ptr(reg), s), "dcv_lecam_apply")
        self.reg = reg
        self.calls += 1

    def compute_dis_losses(self, loss, y_reals: Sequence[torch.Tensor], y_fakes: Sequence[torch.Tensor]):
        """-> one loss per discriminator (loss_idis, loss_vdis, loss_gdis), each `loss.compute_dis_loss(y_real, y_fake)` plus its regulariser term, each carrying
        loss.HostMirroredLoss's host mirror.  Every refusal comes before the first launch."""
        kinds = dis_kinds(loss)
        if len(y_reals) != self.n_dis or len(y_fakes) != self.n_dis:
            raise NativeError(f"LeCam: built for {self.n_dis} discriminators, got {len(y_reals)} real and {len(y_fakes)} fake logit tensors")
        ys = [y for pair in zip(y_reals, y_fakes) for y in pair]
        for i, y in enumerate(ys):
            _require_logits(y, "LeCam: %s logits of discriminator %d" % ("fake" if i % 2 else "real", i // 2))
        if self.state.device.type != "cuda":
            raise NativeError(f"LeCam: the state is on {self.state.device} — the regulariser runs on the GPU only (there is no CPU fallback)")
        return tuple(Lm.HostMirroredLoss.wrap(o) for o in _DisLosses.apply(self, kinds, *ys))

    # ---- host reads: logging and checkpoints only -------------------------------------------------------------------------------------------------------
    def anchors(self) -> torch.Tensor:
        """The device state: (n_dis, 8) int32 — DCV_LECAM_ANCHOR_REAL / _FAKE as fp32 bits, _UPDATES, _ACTIVE (a view; `.view(torch.float32)[:, :2]` are the anchors)."""
        return self.state.view(self.n_dis, STATE_WORDS)

    def state_words(self):
        return [[int(v) for v in row] for row in self.anchors().cpu().tolist()]

    def anchor_values(self):
        """[(aR, aF), ...] as Python floats (a host read)."""
        f = lambda b: struct.unpack("<f", struct.pack("<i", b))[0]
        return [(f(w[ANCHOR_REAL]), f(w[ANCHOR_FAKE])) for w in self.state_words()]

    def state_dict(self):
        return dict(state=self.state_words(), n_dis=self.n_dis, weight=self.weight, decay=self.decay, start=self.start, one_sided=self.one_sided)

    def load_state_dict(self, sd):
        words = [[int(v) for v in row] for row in sd["state"]]
        if len(words) != self.n_dis or any(len(row) != STATE_WORDS for row in words):
            raise ValueError(f"LeCam: the state has {self.n_dis} blocks of {STATE_WORDS} words, the checkpoint {[len(r) for r in words]}")
        self.state.copy_(torch.tensor(words, dtype=torch.int32).reshape(-1))
        self.weight, self.decay, self.start, self.one_sided = float(sd["weight"]), float(sd["decay"]), int(sd["start"]), bool(sd["one_sided"])
