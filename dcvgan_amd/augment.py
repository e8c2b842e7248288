"""Adaptive clip augmentation in front of the discriminators.

A small dataset is memorised by three discriminators long before the generators converge.  The remedy is to augment everything the discriminators see —
the real pair and, differentiably, the fakes — with DiffAugment's transforms (Zhao et al. 2020) at a probability that follows the discriminators' overfitting
(StyleGAN2-ADA, Karras et al. 2020).  Everything here is decided and applied on the device: one ``dcv_aug_draw`` launch makes a (B, 8) int32 parameter table (one
row per clip: all frames and both streams of a pair share it, so depth / flow stays registered with colour and a clip stays consistent in time), one
``dcv_aug_apply`` launch per stream applies it as an exact gather, ``dcv_aug_apply_backward`` is its adjoint, and the probability lives in an 8-word device state
block that ``dcv_aug_observe`` / ``dcv_aug_adjust`` update.  No value is read on the host, no torch kernel runs.  fp32 in, fp32 out.
"""
from __future__ import annotations

import ctypes as C
import math
import struct
from typing import Optional

import torch
from torch.autograd import Function

from . import native as N
from .native import AugLimits, AugWarpLimits, NativeError, check, dims5, lib, ptr, stream_ptr
from .rng import PhiloxRng

FLIP, TRANSLATE, CUTOUT, COLOUR = 1, 2, 4, 8          # dcv_aug_limits.mask
SCALE, ROTATE, ANISO, SUBPIXEL, SATURATION = 16, 32, 64, 128, 256      # dcv_aug_warp_limits.mask: the interpolated warps and saturation
WARP_MASK = SCALE | ROTATE | ANISO | SUBPIXEL | SATURATION
OPS = {"flip": FLIP, "translate": TRANSLATE, "cutout": CUTOUT, "colour": COLOUR,
       "scale": SCALE, "rotate": ROTATE, "aniso": ANISO, "subpixel": SUBPIXEL, "saturation": SATURATION}
ROW_WORDS, WARP_ROW_WORDS = 8, 24                      # a table is (B, 8) with none of the five new ops enabled, else (B, 24)
STATE_WORDS = 8                                        # p (fp32 bits), sum_sign, count, adjusts, 4 reserved
MAX_HW = 4096                                          # the kernels' limit on H and W
IDENTITY_ROW = (0, 0, 0, 0, 0, 0, struct.unpack("<i", struct.pack("<f", 1.0))[0], 0)
_ONE = IDENTITY_ROW[6]
IDENTITY_WARP_ROW = IDENTITY_ROW + (0, _ONE, 0, 0, 0, _ONE, 0, _ONE, 0, 0, _ONE, _ONE, 0, 0, 0, 0)
# The draws' Philox key is the seed plus this constant: a model's latent draw with the same (seed, offset) runs the same counters (idx 0, 1, ..) through another key.
SEED_SALT = 0x9E3779B97F4A7C15


_STATS = {"launches": 0}


def _check_warp_limits(scale_max, aniso_max, rot_max_deg, frac, sat):
    """scale_max * aniso_max <= 2 and |theta| < 180 degrees keep every drawn L inside the adjoint's 9 x 9 candidate box (|l00| + |l01| <= 2 sqrt 2 < 3)."""
    if not (float(scale_max) >= 1.0 and float(aniso_max) >= 1.0 and float(rot_max_deg) >= 0.0 and 0.0 <= float(frac) <= 1.0 and float(sat) >= 0.0):
        raise ValueError(f"ClipAugment: scale_max >= 1, aniso_max >= 1, rot_max_deg >= 0, 0 <= frac <= 1, sat >= 0 (each op's identity or above), got "
                         f"{scale_max!r}, {aniso_max!r}, {rot_max_deg!r}, {frac!r}, {sat!r}")
    if float(scale_max) * float(aniso_max) > 2.0:
        raise ValueError(f"ClipAugment: scale_max * aniso_max must be <= 2 (the adjoint's candidate box), got {scale_max!r} * {aniso_max!r}")
    if float(rot_max_deg) >= 180.0:
        raise ValueError(f"ClipAugment: rot_max_deg must be below 180, got {rot_max_deg!r}")


def launches() -> int:
    """Kernel launches this module has issued so far, in this process (every C entry it calls is one launch): what tests and tools hold the formula of
    ClipAugment.launches_per_iteration against."""
    return _STATS["launches"]


def _call(name: str, *args):
    check(getattr(lib(), name)(*args), name)
    _STATS["launches"] += 1


def _require_clip(t: torch.Tensor, what: str):
    N._require(t, what)        # a HIP device tensor, float32 (a 16-bit tensor is refused), on the current device
    if t.dim() != 5:
        raise NativeError(f"{what}: expected a (B, C, T, H, W) clip, got {tuple(t.shape)}")
    if t.numel() == 0:
        raise NativeError(f"{what}: empty clip")
    if t.shape[3] > MAX_HW or t.shape[4] > MAX_HW:
        raise NativeError(f"{what}: H and W up to {MAX_HW}, got {t.shape[3]} x {t.shape[4]}")


def _require_table(table: torch.Tensor, batch: int, words: int = ROW_WORDS):
    if not table.is_cuda or table.dtype != torch.int32 or tuple(table.shape) != (batch, words) or not table.is_contiguous():
        raise NativeError(f"augmentation table: expected a contiguous ({batch}, {words}) int32 device tensor, got {table.dtype}{tuple(table.shape)} on {table.device}")


def _entry(table: torch.Tensor, what: str) -> str:
    """The C entry for this table's width: dcv_aug_<what> for (B, 8), dcv_aug_warp_<what> for (B, 24).  The last integer argument of an entry is
    flip_negate_channel for the first family and vector_channels for the second."""
    return ("dcv_aug_warp_" if table.shape[1] == WARP_ROW_WORDS else "dcv_aug_") + what


def _launch(fn_name: str, x: torch.Tensor, table: torch.Tensor, colour: bool, neg_ch: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    y = torch.empty(tuple(x.shape), dtype=torch.float32, device=x.device) if out is None else out
    xd, yd = dims5(x), dims5(y)
    _call(fn_name, ptr(x), C.byref(xd), ptr(table), int(table.shape[0]), ptr(y), C.byref(yd), int(colour), int(neg_ch), stream_ptr())
    return y


def _layout_of(shape, strides):
    """What a gradient of a tensor with this shape and these strides is written into: the tensor's own layout when it is a dense permutation — the generators'
    clips are (B, T, C, H, W) memory viewed as (B, C, T, H, W), and the view chain back into the generator then needs no copy — else contiguous."""
    order = sorted(range(len(shape)), key=lambda i: -strides[i])
    want, dense = 1, True
    for i in reversed(order):
        if shape[i] != 1 and strides[i] != want:
            dense = False
        want *= shape[i]
    return tuple(strides) if dense else None


def _grad_like(shape, strides, device) -> torch.Tensor:
    if strides is None:
        return torch.empty(tuple(shape), dtype=torch.float32, device=device)
    return torch.empty_strided(tuple(shape), strides, dtype=torch.float32, device=device)


def apply(x: torch.Tensor, table: torch.Tensor, colour: bool, flip_negate_channel: int = -1) -> torch.Tensor:
    """One stream's forward without a tape: dcv_aug_apply."""
    _require_clip(x, "augment input")
    _require_table(table, x.shape[0])
    return _launch("dcv_aug_apply", x, table, colour, flip_negate_channel)


def apply_backward(dy: torch.Tensor, table: torch.Tensor, colour: bool, flip_negate_channel: int = -1, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One stream's adjoint: dcv_aug_apply_backward (into `out`, a strided view of dy's shape, or a fresh contiguous tensor)."""
    _require_clip(dy, "augment cotangent")
    _require_table(table, dy.shape[0])
    return _launch("dcv_aug_apply_backward", dy, table, colour, flip_negate_channel, out)


def warp_apply(x: torch.Tensor, table: torch.Tensor, colour: bool, vector_channels: int = 0) -> torch.Tensor:
    """One stream's forward under a (B, 24) table without a tape: dcv_aug_warp_apply."""
    _require_clip(x, "augment input")
    _require_table(table, x.shape[0], WARP_ROW_WORDS)
    _require_streams(colour, vector_channels)
    return _launch("dcv_aug_warp_apply", x, table, colour, vector_channels)


def warp_apply_backward(dy: torch.Tensor, table: torch.Tensor, colour: bool, vector_channels: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One stream's adjoint under a (B, 24) table: dcv_aug_warp_apply_backward (into `out`, a strided view of dy's shape, or a fresh contiguous tensor)."""
    _require_clip(dy, "augment cotangent")
    _require_table(table, dy.shape[0], WARP_ROW_WORDS)
    _require_streams(colour, vector_channels)
    return _launch("dcv_aug_warp_apply_backward", dy, table, colour, vector_channels, out)


def _require_streams(colour, vector_channels):
    if int(vector_channels) not in (0, 1) or (colour and vector_channels):
        raise NativeError(f"augment: vector_channels is 0 or 1, and 0 on the colour stream (got {vector_channels!r}, colour {colour!r})")


def _adjoint(dy, table, colour, ch, out):
    return _launch(_entry(table, "apply_backward"), dy, table, colour, ch, out)


class _AugPair(Function):
    """(xg, xc) -> (yg, yc) under one table.  The backward launches one adjoint per stream that received a cotangent and whose input asked for a gradient, and
    writes each gradient in its input's own layout."""

    @staticmethod
    def forward(ctx, xg, xc, table, neg_g, neg_c):
        ctx.table, ctx.neg = table, (int(neg_g), int(neg_c))
        ctx.layouts = [(tuple(x.shape), _layout_of(tuple(x.shape), tuple(x.stride()))) for x in (xg, xc)]
        ctx.set_materialize_grads(False)
        return _launch(_entry(table, "apply"), xg, table, False, neg_g), _launch(_entry(table, "apply"), xc, table, True, neg_c)

    @staticmethod
    def backward(ctx, dyg, dyc):
        from .ops import _dense
        dg = dc = None
        if dyg is not None and ctx.needs_input_grad[0]:
            dg = _adjoint(_dense(dyg), ctx.table, False, ctx.neg[0], _grad_like(*ctx.layouts[0], dyg.device))
        if dyc is not None and ctx.needs_input_grad[1]:
            dc = _adjoint(_dense(dyc), ctx.table, True, ctx.neg[1], _grad_like(*ctx.layouts[1], dyc.device))
        return dg, dc, None, None, None


class _AugOne(Function):
    """One stream of a pair under a table made earlier (the fakes' colour clip only exists after the colour generator has read the geometry clip)."""

    @staticmethod
    def forward(ctx, x, table, colour, neg):
        ctx.table, ctx.colour, ctx.neg = table, bool(colour), int(neg)
        ctx.layout = (tuple(x.shape), _layout_of(tuple(x.shape), tuple(x.stride())))
        return _launch(_entry(table, "apply"), x, table, colour, neg)

    @staticmethod
    def backward(ctx, dy):
        from .ops import _dense
        return _adjoint(_dense(dy), ctx.table, ctx.colour, ctx.neg, _grad_like(*ctx.layout, dy.device)), None, None, None


class _AugFan(Function):
    """The fakes' geometry clip x and its four readers (trainer.py:303-309, 344-349): the colour generator reads x as it is, the video and the gradient discriminator
    read the augmented clip y, the image discriminator frame `t` of y.  Outputs: (x, y[:, :, t], y, y) as views.  The backward forms x's ONE gradient
        ((d_cgen + A^T d_vdis) + A^T d_gdis) + A^T embed_t(d_idis)
    in one dcv_aug_fan_backward launch, in x's own layout.  Under the identity row A^T moves bits, and this is the sum ops.fan_out forms without the augmentation,
    addition for addition: an augmentation at p = 0 leaves every gradient bit where it was."""

    @staticmethod
    def forward(ctx, x, table, neg, t):
        ctx.table, ctx.neg, ctx.t = table, int(neg), int(t)
        ctx.layout = (tuple(x.shape), _layout_of(tuple(x.shape), tuple(x.stride())))
        ctx.set_materialize_grads(False)
        y = _launch(_entry(table, "apply"), x, table, False, neg)
        return x.view_as(x), y[:, :, ctx.t], y.view_as(y), y.view_as(y)

    @staticmethod
    def backward(ctx, d_c, d_f, d_v, d_g):
        from .ops import _dense
        full = [_dense(g) for g in (d_v, d_g) if g is not None]
        if d_c is None and d_f is None and not full:
            return None, None, None, None
        if not full and d_f is None:
            return d_c, None, None, None      # only the un-augmented reader delivered a gradient
        ref = full[0] if full else d_f
        for g in full + ([d_c] if d_c is not None else []) + ([d_f] if d_f is not None else []):
            N._require(g, "augment cotangent")
        out = _grad_like(*ctx.layout, ref.device)
        d_f = None if d_f is None else _dense(d_f).unsqueeze(2)
        d_c = None if d_c is None else _dense(d_c)
        dd = lambda g: (ptr(g), C.byref(dims5(g))) if g is not None else (None, None)
        g0, g1 = (full + [None, None])[:2]
        od = dims5(out)
        _call(_entry(ctx.table, "fan_backward"), *dd(d_c), *dd(g0), *dd(g1), *dd(d_f), ctx.t, ptr(ctx.table), int(ctx.table.shape[0]), ptr(out), C.byref(od), 0, ctx.neg,
              stream_ptr())
        return out, None, None, None


class ClipAugment:
    """``aug = ClipAugment(cfg, device, p=0.0, adaptive=True)``; ``yg, yc = aug(xg, xc)`` for the real pair and for each phase's fakes.

    ``adaptive=True``: ``aug.observe(y_real)`` for each discriminator's real logits and ``aug.end_of_iteration(i)`` once per iteration; every ``interval``
    iterations p moves by ``step = batch * interval / adjust_clips`` towards keeping r = E[sign(D(real))] at ``target``, inside [0, p_max].  The defaults
    (target 0.6, interval 4, p_max 0.8, adjust_clips 500 000) are StyleGAN2-ADA's published values for images; nobody has tuned them for clips.
    ``adaptive=False, p=<value>``: a fixed probability (p = 1.0 is DiffAugment); observe / adjust are never launched.
    ``ops``: the enabled transforms, any of "flip", "translate", "cutout", "colour".  ``max_dx`` / ``max_dy`` / ``cut_size`` default to W/8, H/8 and min(H, W)/2 of
    the clip at hand; ``contrast`` 0.5 (gain in (0.5, 1.5]) and ``brightness`` 1.0 (bias in (-0.5, 0.5]) are DiffAugment's.
    The geometry stream of an optical-flow config negates channel 0 (the horizontal component) under a flip.
    Interpolated warps and saturation, off unless named in ``ops``: "scale" (isotropic, ratio in [1/scale_max, scale_max]), "rotate" (up to
    ``rot_max_deg`` either way; the draw is uniform in tan(theta / 2), so theta is slightly denser towards 0), "aniso" (sx / sy ratio up to aniso_max^2),
    "subpixel" (a shift of up to ``frac`` of the plane on top of the integer one), "saturation" (about the pixel's channel mean, s in 1 + sat * (-1, 1]; RGB only).
    The defaults (1.3, 45, 1.25, 0.125, 1.0) are ADA-like; nobody has tuned them for clips.  With any of the five enabled the table is (B, 24) and the
    dcv_aug_warp_* entries run — bilinear taps, a gather adjoint, still no atomics and no torch kernel; an optical-flow clip's vectors turn with the warp.
    With none enabled nothing changes: the (B, 8) table, the same entries, the same draws, the same state_dict keys.
    The draws come from a PhiloxRng of this object's own: the models' random streams are what they are without augmentation.
    Data parallel: with torch.distributed initialised and more than one rank, the two accumulators are all-reduced (SUM, int32: exact, order-free) over a process
    group of this object's own before every adjustment, so every rank holds the same p.  Constructing it is then a collective call."""

    def __init__(self, cfg, device, p: float = 0.0, adaptive: bool = True, target: float = 0.6, interval: int = 4, p_max: float = 0.8,
                 adjust_clips: int = 500_000, ops=("flip", "translate", "cutout", "colour"), max_dx: Optional[int] = None, max_dy: Optional[int] = None,
                 cut_size: Optional[int] = None, contrast: float = 0.5, brightness: float = 1.0, batch: Optional[int] = None, seed: Optional[int] = None,
                 scale_max: float = 1.3, aniso_max: float = 1.25, rot_max_deg: float = 45.0, frac: float = 0.125, sat: float = 1.0):
        if not 0.0 <= float(p) <= 1.0 or not 0.0 <= float(p_max) <= 1.0:
            raise ValueError(f"ClipAugment: p and p_max must be in [0, 1], got {p!r}, {p_max!r}")
        if not -1.0 <= float(target) <= 1.0 or int(interval) < 1 or int(adjust_clips) < 1 or contrast < 0 or brightness < 0:
            raise ValueError("ClipAugment: target in [-1, 1], interval >= 1, adjust_clips >= 1, contrast >= 0, brightness >= 0")
        unknown = [o for o in ops if o not in OPS]
        if unknown:
            raise ValueError(f"ClipAugment: unknown ops {unknown}; known: {sorted(OPS)}")
        _check_warp_limits(scale_max, aniso_max, rot_max_deg, frac, sat)
        self.scale_max, self.aniso_max, self.rot_max_deg, self.frac, self.sat = float(scale_max), float(aniso_max), float(rot_max_deg), float(frac), float(sat)
        self.cfg, self.device = cfg, torch.device(device)
        self.adaptive, self.target, self.interval, self.p_max, self.adjust_clips = bool(adaptive), float(target), int(interval), float(p_max), int(adjust_clips)
        self.batch = int(batch if batch is not None else cfg.batchsize)
        self.mask = 0
        for o in ops:
            self.mask |= OPS[o]
        self.max_dx, self.max_dy, self.cut_size, self.contrast, self.brightness = max_dx, max_dy, cut_size, float(contrast), float(brightness)
        self.neg_g = 0 if getattr(cfg, "geometric_info", None) == "optical-flow" else -1      # a mirrored flow field's horizontal component changes sign
        self.neg_c = -1
        self.vector_channels = 1 if self.neg_g == 0 else 0      # what the (B, 24) entries take in flip_negate_channel's place
        self.rng = PhiloxRng(seed)
        # the state block: a host tensor copied to the device once (no kernel)
        self.state = self._host_state(float(p), 0, 0, 0).to(self.device)
        self.pg, self.world = None, 1
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            self.pg, self.world = dist.new_group(), dist.get_world_size()
        self.draws = 0      # counters for tests / tools
        self.collectives = 0

    @staticmethod
    def _host_state(p, sum_sign, count, adjusts) -> torch.Tensor:
        bits = struct.unpack("<i", struct.pack("<f", p))[0]
        return torch.tensor([bits, int(sum_sign), int(count), int(adjusts), 0, 0, 0, 0], dtype=torch.int32)

    @property
    def step(self) -> float:
        """p's move per adjustment: batch * interval / adjust_clips in double; the C entry takes it rounded to fp32."""
        return self.batch * self.interval / self.adjust_clips

    def limits(self, H: int, W: int) -> AugLimits:
        return AugLimits(int(self.max_dx if self.max_dx is not None else W // 8), int(self.max_dy if self.max_dy is not None else H // 8),
                         int(self.cut_size if self.cut_size is not None else min(H, W) // 2), self.mask & 15, self.contrast, self.brightness)

    @property
    def warp(self) -> bool:
        """Any of scale / rotate / aniso / subpixel / saturation enabled: the (B, 24) table and the dcv_aug_warp_* entries."""
        return bool(self.mask & WARP_MASK)

    @property
    def row_words(self) -> int:
        return WARP_ROW_WORDS if self.warp else ROW_WORDS

    def warp_limits(self) -> AugWarpLimits:
        return AugWarpLimits(self.scale_max, self.aniso_max, math.tan(math.radians(self.rot_max_deg) / 2.0), self.frac, self.sat, self.mask & WARP_MASK)

    def _channels(self):
        """(geometry, colour): the entries' last integer argument for this object's table width."""
        return (self.vector_channels, 0) if self.warp else (self.neg_g, self.neg_c)

    def draw(self, B: int, H: int, W: int) -> torch.Tensor:
        """A fresh (B, 8) — with a warp op enabled (B, 24) — table at the state block's current p: one launch, and one step of this object's random stream."""
        if self.state.device.type != "cuda":
            raise NativeError(f"ClipAugment: the state block is on {self.state.device} — the augmentation runs on the GPU only (there is no CPU fallback)")
        table = torch.empty((int(B), self.row_words), dtype=torch.int32, device=self.state.device)
        lim = self.limits(H, W)
        seed, offset = self.rng._next()
        if self.warp:
            wl = self.warp_limits()
            _call("dcv_aug_warp_draw", ptr(table), int(B), int(H), int(W), ptr(self.state), C.byref(lim), C.byref(wl), (seed + SEED_SALT) & 0xFFFFFFFFFFFFFFFF, offset,
                  stream_ptr())
            self.draws += 1
            return table
        _call("dcv_aug_draw", ptr(table), int(B), int(H), int(W), ptr(self.state), C.byref(lim), (seed + SEED_SALT) & 0xFFFFFFFFFFFFFFFF, offset, stream_ptr())
        self.draws += 1
        return table

    def __call__(self, xg: torch.Tensor, xc: torch.Tensor, table: Optional[torch.Tensor] = None):
        """(yg, yc): both streams of a pair under one table — drawn here, or injected (tests).  Every refusal comes before the first launch."""
        _require_clip(xg, "augment geometry clip")
        _require_clip(xc, "augment colour clip")
        if xg.shape[0] != xc.shape[0] or tuple(xg.shape[2:]) != tuple(xc.shape[2:]):
            raise NativeError(f"augment: the pair's clips differ in B, T, H or W: {tuple(xg.shape)} and {tuple(xc.shape)}")
        B, H, W = xg.shape[0], xg.shape[3], xg.shape[4]
        if table is not None:
            _require_table(table, B, self.row_words)
        else:
            table = self.draw(B, H, W)
        ch_g, ch_c = self._channels()
        if torch.is_grad_enabled() and (xg.requires_grad or xc.requires_grad):
            return _AugPair.apply(xg, xc, table, ch_g, ch_c)
        # nothing asks for a gradient: no tape entry
        return _launch(_entry(table, "apply"), xg, table, False, ch_g), _launch(_entry(table, "apply"), xc, table, True, ch_c)

    def fan_geometry(self, xg: torch.Tensor, t: int, table: torch.Tensor):
        """The fakes' geometry clip under a tape -> (xg for the colour generator, frame t / whole / whole of the augmented clip for the three discriminators); the
        gradient fan-in of all four readers is one launch (_AugFan)."""
        _require_clip(xg, "augment geometry clip")
        _require_table(table, xg.shape[0], self.row_words)
        if not 0 <= int(t) < xg.shape[2]:
            raise NativeError(f"augment: frame {t} of a clip of {xg.shape[2]}")
        return _AugFan.apply(xg, table, self._channels()[0], int(t))

    def colour(self, xc: torch.Tensor, table: torch.Tensor) -> torch.Tensor:
        """The colour clip of the pair whose geometry clip went through fan_geometry with the same table."""
        _require_clip(xc, "augment colour clip")
        _require_table(table, xc.shape[0], self.row_words)
        if torch.is_grad_enabled() and xc.requires_grad:
            return _AugOne.apply(xc, table, True, self._channels()[1])
        return _launch(_entry(table, "apply"), xc, table, True, self._channels()[1])

    def observe(self, y: torch.Tensor):
        """Add a discriminator's logits on the real batch to the accumulators (adaptive mode; a no-op in fixed mode)."""
        if not self.adaptive:
            return
        y = y.detach()
        N._require(y, "augment.observe logits")
        if not y.is_contiguous() or y.numel() < 1:
            raise NativeError("augment.observe: expected a non-empty contiguous logit tensor")
        _call("dcv_aug_observe", ptr(y), y.numel(), ptr(self.state), stream_ptr())

    def adjust(self):
        """One adjustment now (end_of_iteration calls it at interval boundaries)."""
        if self.world > 1:
            import torch.distributed as dist
            dist.all_reduce(self.state[1:3], op=dist.ReduceOp.SUM, group=self.pg)
            self.collectives += 1
        _call("dcv_aug_adjust", ptr(self.state), self.target, self.step, self.p_max, stream_ptr())

    def end_of_iteration(self, iteration: int):
        """`iteration` counts from 1.  The host knows the iteration number; nothing is read back."""
        if self.adaptive and int(iteration) % self.interval == 0:
            self.adjust()

    def launches_per_iteration(self, iteration: int, taped_phases: int) -> int:
        """Launches the augmentation adds to iteration `iteration` of StepRunner: 3 draws + 6 applies + 2 adjoints per phase whose fakes carry a tape (and whose
        backward runs) + in adaptive mode 3 observes + 1 adjust at an interval boundary."""
        n = 3 + 6 + 2 * int(taped_phases)
        if self.adaptive:
            n += 3 + (1 if int(iteration) % self.interval == 0 else 0)
        return n

    # ---- host reads: logging and checkpoints only -------------------------------------------------------------------------------------------------------
    def state_words(self):
        return [int(v) for v in self.state.cpu().tolist()]

    def p(self) -> float:
        return struct.unpack("<f", struct.pack("<i", self.state_words()[0]))[0]

    def adjusts(self) -> int:
        return self.state_words()[3]

    def state_dict(self):
        sd = self._state_dict_v1()
        if self.warp:      # (today's keys only without a warp op)
            sd.update(scale_max=self.scale_max, aniso_max=self.aniso_max, rot_max_deg=self.rot_max_deg, frac=self.frac, sat=self.sat)
        return sd

    def _state_dict_v1(self):
        return dict(state=self.state_words(), adaptive=self.adaptive, target=self.target, interval=self.interval, p_max=self.p_max, adjust_clips=self.adjust_clips,
                    batch=self.batch, mask=self.mask, max_dx=self.max_dx, max_dy=self.max_dy, cut_size=self.cut_size, contrast=self.contrast,
                    brightness=self.brightness, rng=dict(fixed_seed=self.rng._fixed_seed, seed_seen=self.rng._seed_seen, counter=self.rng._counter))

    def load_state_dict(self, sd):
        words = [int(v) for v in sd["state"]]
        if len(words) != STATE_WORDS:
            raise ValueError(f"ClipAugment: the state block has {STATE_WORDS} words, the checkpoint {len(words)}")
        # the warp constants and the mask are held to the constructor's refusals before anything of this object changes
        warp = {k: float(sd.get(k, getattr(self, k))) for k in ("scale_max", "aniso_max", "rot_max_deg", "frac", "sat")}
        _check_warp_limits(**warp)
        if int(sd["mask"]) & ~(15 | WARP_MASK):
            raise ValueError(f"ClipAugment: the checkpoint's mask {sd['mask']!r} has bits of no known op")
        self.state.copy_(torch.tensor(words, dtype=torch.int32))
        self.adaptive, self.target, self.interval, self.p_max = bool(sd["adaptive"]), float(sd["target"]), int(sd["interval"]), float(sd["p_max"])
        self.adjust_clips, self.batch, self.mask = int(sd["adjust_clips"]), int(sd["batch"]), int(sd["mask"])
        self.max_dx, self.max_dy, self.cut_size = sd["max_dx"], sd["max_dy"], sd["cut_size"]
        self.contrast, self.brightness = float(sd["contrast"]), float(sd["brightness"])
        for k, v in warp.items():      # a checkpoint without them loads: the constructor's values stay
            setattr(self, k, v)
        r = sd["rng"]
        self.rng._fixed_seed, self.rng._seed_seen, self.rng._counter = r["fixed_seed"], r["seed_seen"], int(r["counter"])
