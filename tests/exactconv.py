"""Host side of the exact-integer convolution checks (tests/test_conv_exact_cpu.py, tests/test_conv_exact_gpu.py).  No GPU is touched here.

A convolution is a sum of products.  With small-integer operands every product and every partial sum is an integer below 2^24, whatever the order, tiling,
split-K, slab reduce or two-level accumulation: all of them are exact in fp32, so a kernel's result must equal the fp64 host convolution bit for bit, and one
mis-indexed tap, tile edge or slab shows as a non-zero integer difference at a known index.  This module makes the operands, computes the reference, checks
the conditions under which "exact" holds (from the operands and the reference alone), and describes a mismatch by its coordinates."""
import functools
import time
import zlib
from collections import namedtuple

import torch
import torch.nn.functional as F

SLOPE = 0.25                      # a power of two: leaky(y) of an integer y is exact in fp32 and in 16 bits
EXACT = 1 << 24                   # every integer of magnitude <= 2^24 is an fp32 value
HALF_EXACT = {torch.bfloat16: 256, torch.float16: 2048}      # ... 2^8 a bf16 value, 2^11 an fp16 value
FP64_BUDGET_MACS = 6e9            # beyond this many multiply-adds (about 5 s of fp64 host time for the three passes) the fp32 host convolution is the reference:
                                  # under the reduction bound it is exact as well (test_conv_exact_cpu.py checks that claim)

# name, transposed, dims, cin, cout, kernel, stride, padding, input spatial, samples, operand magnitude, operand density
Case = namedtuple("Case", "name tr nd cin cout k s p sp n mag density")


def case(name, tr, nd, cin, cout, k, s, p, sp, n, mag=2, density=1.0):
    return Case(name, bool(tr), nd, cin, cout, k, s, p, tuple(sp), n, mag, density)


def _t(v, nd):
    return (v,) * nd if isinstance(v, int) else tuple(v)


def seed_of(name):
    """The same seed in every process (str hashes are salted per process: a failing case could not be reproduced from its id)."""
    return zlib.crc32(name.encode())


def int_operands(shape, magnitude, density, seed):
    """fp32 tensor of integers uniform in [-magnitude, magnitude], zeroed with probability 1 - density"""
    g = torch.Generator().manual_seed(seed)
    v = torch.randint(-magnitude, magnitude + 1, tuple(shape), generator=g).float()
    if density < 1.0:
        v = v * (torch.rand(tuple(shape), generator=g) < density).float()
    return v


def conv_fn(c):
    return {(False, 2): F.conv2d, (False, 3): F.conv3d, (True, 2): F.conv_transpose2d, (True, 3): F.conv_transpose3d}[(c.tr, c.nd)]


def weight_shape(c):
    return ((c.cin, c.cout) if c.tr else (c.cout, c.cin)) + _t(c.k, c.nd)


def out_spatial(c):
    k, s, p = _t(c.k, c.nd), _t(c.s, c.nd), _t(c.p, c.nd)
    return tuple((i - 1) * st - 2 * pd + kk if c.tr else (i + 2 * pd - kk) // st + 1 for i, kk, st, pd in zip(c.sp, k, s, p))


def leaky(y, slope=SLOPE):
    return torch.where(y > 0, y, y * slope)


def macs(c):
    taps = 1
    for v in _t(c.k, c.nd):
        taps *= v
    pos = c.n
    for v in (c.sp if c.tr else out_spatial(c)):
        pos *= v
    return 3.0 * pos * c.cin * c.cout * taps


@functools.lru_cache(maxsize=4)
def reference(c):
    """Everything a device result of this convolution is compared with, in fp64 on the host (computed once per case and shared by its passes and precisions:
    leave it unchanged).  x, w, dy: the fp32 operands.  old / old_dw / xg: what the accumulating and the gated entries start from."""
    t0 = time.time()
    sd = seed_of(c.name)
    x = int_operands((c.n, c.cin) + c.sp, c.mag, c.density, sd)
    w = int_operands(weight_shape(c), c.mag, c.density, sd + 1)
    dy = int_operands((c.n, c.cout) + out_spatial(c), c.mag, c.density, sd + 2)
    old = int_operands(x.shape, 8, 1.0, sd + 3)
    xg = int_operands(x.shape, 3, 1.0, sd + 4)
    old_dw = int_operands(w.shape, 8, 1.0, sd + 5)
    wide = macs(c) <= FP64_BUDGET_MACS
    dt = torch.float64 if wide else torch.float32
    xr, wr = x.clone().to(dt).requires_grad_(True), w.clone().to(dt).requires_grad_(True)
    y = conv_fn(c)(xr, wr, None, _t(c.s, c.nd), _t(c.p, c.nd))
    dx, dw = torch.autograd.grad((y * dy.to(dt)).sum(), [xr, wr])
    y, dx, dw = y.detach().double(), dx.double(), dw.double()
    red = tuple(i for i in range(y.dim()) if i != 1)
    r = dict(x=x, w=w, dy=dy, old=old, xg=xg, old_dw=old_dw, y=y, dx=dx, dw=dw, host_dtype=dt,
             y_leaky=leaky(y), dx_acc=old.double() + dx, dx_gated=(old.double() + dx) * torch.where(xg > 0, 1.0, SLOPE).double(),
             dx_gated_plain=dx * torch.where(xg > 0, 1.0, SLOPE).double(), dw_acc=old_dw.double() + dw,
             sum_y=y.sum(red), sum_y2=(y * y).sum(red))
    r["seconds"] = time.time() - t0
    return r


def thin_z(c, r, which):
    """The 16-bit intermediate of the channels-last path's thin-destination form (tests/test_cl16_plan_cpu.py: the Z tensor): a 1 x 1 GEMM over the SOURCE
    channels, per tap and destination channel, before the taps of a destination pixel are gathered.  which 0: forward (source x), 1: data gradient (source dy).
    Returns max |Z|."""
    w = r["w"].double().flatten(2)                                   # (a, b, taps)
    forward_reads_first = (which == 0) == (not c.tr)                 # conv forward / convT data gradient reduce over the weight's SECOND axis
    src = (r["x"] if which == 0 else r["dy"]).double().flatten(2)    # (n, source channels, pixels)
    z = torch.einsum("ncp,dct->ndtp", src, w) if forward_reads_first else torch.einsum("ncp,cdt->ndtp", src, w)
    return float(z.abs().max())


def assert_exactness_bounds(c, r, half=None, stats=False):
    """Conditions (not tolerances) under which the device result must equal the reference bit for bit; checked from the operands and the reference alone,
    before any device result is looked at.  half: torch.bfloat16 / torch.float16 for the channels-last path.  stats: the case runs a fused BatchNorm-sums entry."""
    taps = 1
    for v in _t(c.k, c.nd):
        taps *= v
    mx, mw, mdy = float(r["x"].abs().max()), float(r["w"].abs().max()), float(r["dy"].abs().max())
    K_fwd, K_bwd = c.cin * taps, c.cout * taps      # the forward reduces over (cin, taps), the data gradient over (cout, taps), transposed or not
    M = c.n                                         # the weight gradient over the positions of the dense operand
    for v in (c.sp if c.tr else out_spatial(c)):
        M *= v
    # reduction bound: from the definition of the sums
    assert K_fwd * mx * mw < EXACT, (c.name, "forward reduction", K_fwd, mx, mw)
    assert K_bwd * mdy * mw < EXACT, (c.name, "data-gradient reduction", K_bwd, mdy, mw)
    assert M * mx * mdy < EXACT, (c.name, "weight-gradient reduction", M, mx, mdy)
    # accumulate variants
    assert float(r["old"].abs().max()) + K_bwd * mdy * mw < EXACT and float(r["old"].abs().max()) + float(r["dx"].abs().max()) < EXACT, (c.name, "accumulated dx")
    assert float(r["old_dw"].abs().max()) + M * mx * mdy < EXACT, (c.name, "accumulated dw")
    # the operands themselves are integers, and 16-bit exact where the path stores them in 16 bits
    for key in ("x", "w", "dy", "old", "xg", "old_dw"):
        assert bool((r[key] == r[key].round()).all()), (c.name, key)
    if stats:
        red = tuple(i for i in range(r["y"].dim()) if i != 1)
        assert float(r["y"].abs().sum(red).max()) < EXACT and float(r["sum_y2"].max()) < EXACT, (c.name, "BatchNorm partial sums", float(r["sum_y2"].max()))
    if half is not None:
        lim = HALF_EXACT[half]
        assert max(mx, mw, mdy, float(r["old"].abs().max()), float(r["xg"].abs().max())) <= lim, (c.name, "16-bit operands")
        # a thin destination (<= 8 channels) may run as a 1x1 GEMM whose 16-bit result Z is gathered afterwards: Z must be exact in 16 bits
        if c.cout <= 8:
            assert thin_z(c, r, 0) <= lim, (c.name, "Z of the forward", thin_z(c, r, 0), lim)
        if c.cin <= 8:
            assert thin_z(c, r, 1) <= lim, (c.name, "Z of the data gradient", thin_z(c, r, 1), lim)


def first_mismatch(got, want, tile=128, limit=6):
    """'' when got equals want; else the count of differing elements, the first few as (n, c, d, h, w): got, want, and where they lie: on the tensor's border
    rows / columns, on its last channel tile (channels >= the last multiple of `tile`), on its last sample."""
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    assert got.shape == want.shape, (got.shape, want.shape)
    g5 = got.reshape(got.shape[:2] + (1,) * (5 - got.dim()) + got.shape[2:]) if got.dim() < 5 else got
    w5 = want.reshape(g5.shape)
    bad = ~((g5 == w5) | (torch.isnan(g5) & torch.isnan(w5)))
    nbad = int(bad.sum())
    if nbad == 0:
        return ""
    idx = bad.nonzero()
    N, Cc, D, H, W = g5.shape
    border = ((idx[:, 3] == 0) | (idx[:, 3] == H - 1) | (idx[:, 4] == 0) | (idx[:, 4] == W - 1))
    last_tile = idx[:, 1] >= (Cc - 1) // tile * tile
    last_n = idx[:, 0] == N - 1
    lines = [f"{nbad} of {bad.numel()} elements differ; on border rows/columns: {int(border.sum())}, on the last channel tile (c >= {(Cc - 1) // tile * tile}): "
             f"{int(last_tile.sum())}, on the last sample: {int(last_n.sum())}"]
    for i in idx[:limit].tolist():
        lines.append(f"  (n, c, d, h, w) = {tuple(i)}: got {float(g5[tuple(i)])!r}, want {float(w5[tuple(i)])!r}")
    return "\n".join(lines)


def assert_equal(got, want, what):
    """torch.equal, with the coordinates of the first differences in the failure message"""
    got = got.detach().cpu()
    want = want.detach().cpu()
    if got.dtype != want.dtype or not torch.equal(got, want):
        msg = first_mismatch(got, want)
        assert got.dtype == want.dtype and torch.equal(got, want), f"{what}: {msg}"
