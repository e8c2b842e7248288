"""Host side of the exact-integer BatchNorm checks (tests/test_bn_exact_cpu.py, tests/test_bn_exact_gpu.py).  No GPU is touched here.

A BatchNorm reduction is a sum and its apply passes are a few multiply-adds.  With x = m_c +- a_c (m_c an integer, a_c a power of two, as many + as - per
channel) sum x = m count and sum x^2 = (m^2 + a^2) count are integers, every fp32 run the kernels make stays far below 2^24, mean = m and var = a^2 come out
exactly in the kernels' fp64, and with eps = 0 invstd = 1 / a.  gamma a power of two, beta an integer, dy an integer, a dropout mask in {0, 2} and a LeakyReLU slope
of 1/4 keep y, dz, sum dz and sum dz xhat exact as well.  One dropped, doubled or mis-addressed element is then a non-zero difference at a known index, whatever
the size of the tensor.  This module makes the operands, computes the fp64 reference, decides FROM THE OPERANDS AND THE REFERENCE ALONE which quantities are exact
(and bounds the others by counting roundings), copies the dispatch arithmetic of csrc/elementwise.hip and csrc/cl_elementwise.hip, and describes a mismatch by its
coordinates and by the block / segment / slot / row that owns it."""
import math
import zlib
from collections import namedtuple

import torch

SLOPE = 0.25                      # a power of two
U = 2.0 ** -24                    # fp32 unit roundoff
GUARD = 8192                      # NaN elements on either side of every operand
RUN32, RUN_SMALL, RUN_CL = 256, 32, 64      # longest fp32 run (terms) before a kernel folds into fp64: bn_stats / bn_bwd_reduce (64 trips x 4), small kernels, CL kernels
MODES = ("leaky", "dropout", "none", "eval")


def seed_of(name):
    return zlib.crc32(name.encode())


def five(shape):
    """(N, C, H, W) or (N, C, D, H, W) -> (N, C, D, H, W)"""
    return tuple(shape) if len(shape) == 5 else (shape[0], shape[1], 1) + tuple(shape[2:])


# ------------------------------------------------------------------------------------------------------------------------------------------------------
# layouts of the fp32 path: every operand is torch.as_strided(storage, shape, strides, GUARD + offset) inside a NaN-guarded allocation
# ------------------------------------------------------------------------------------------------------------------------------------------------------
def layout_of(shape, layout):
    """-> (element strides of the 5-D view, offset of its first element in the body, body elements).  `layout` is a name or ("slice", total channels, first channel)."""
    N, C, D, H, W = five(shape)
    hw, dhw = H * W, D * H * W
    if layout == "plain":
        return (C * dhw, dhw, hw, W, 1), 0, N * C * dhw
    if layout == "misaligned":                 # the first element 4 bytes past a 16-byte boundary
        return (C * dhw, dhw, hw, W, 1), 1, N * C * dhw + 1
    if layout == "nstride2":                   # two spare elements after every sample
        return (C * dhw + 2, dhw, hw, W, 1), 0, N * (C * dhw + 2)
    if layout == "wstep2":                     # big[..., ::2]
        return (C * dhw * 2, dhw * 2, hw * 2, W * 2, 2), 0, N * C * dhw * 2
    if layout == "hw_transposed":              # a (N, C, D, W, H) tensor seen as (N, C, D, H, W)
        return (C * dhw, dhw, hw, 1, H), 0, N * C * dhw
    if layout == "permuted":                   # permute(0, 2, 1, 3, 4) of a contiguous (B, T, C, H, W): the generators' layout
        return (D * C * hw, hw, C * hw, W, 1), 0, N * C * dhw
    if isinstance(layout, tuple) and layout[0] == "slice":      # channels [c0, c0 + C) of a buffer with `total` channels: ConcatBuffer
        total, c0 = layout[1], layout[2]
        return (total * dhw, dhw, hw, W, 1), c0 * dhw, N * total * dhw
    raise ValueError(layout)


def view_in(storage, shape, layout):
    st, off, _ = layout_of(shape, layout)
    if len(shape) == 4:
        st = st[:2] + st[3:]
    return torch.as_strided(storage, tuple(shape), st, GUARD + off)


def guarded(shape, layout, device, fill=None, body=float("nan"), dtype=torch.float32):
    """A view of `shape` in `layout` inside an allocation with GUARD NaNs on either side; the body outside the view holds `body`.  -> (view, storage)"""
    _, _, n = layout_of(shape, layout)
    storage = torch.full((n + 2 * GUARD,), float("nan"), dtype=dtype, device=device)
    storage[GUARD:GUARD + n] = body
    v = view_in(storage, shape, layout)
    if fill is not None:
        v.copy_(fill)
    return v, storage


def untouched_outside(storage, before, shape, layout):
    """True iff `storage` equals its snapshot `before` bit for bit everywhere outside the view (guard bands and the rest of the body)"""
    a, b = storage.clone(), before.clone()
    view_in(a, shape, layout).zero_()
    view_in(b, shape, layout).zero_()
    it = {4: torch.int32, 2: torch.int16}[a.element_size()]
    return bool(torch.equal(a.view(it), b.view(it)))


# ------------------------------------------------------------------------------------------------------------------------------------------------------
# the dispatch arithmetic of csrc/elementwise.hip (make_rowmap, make_chanmap, bn_small_ok, launch_ew) — the tests' own copy
# ------------------------------------------------------------------------------------------------------------------------------------------------------
Dispatch = namedtuple("Dispatch", "vec inner gpr groups per_chan split seg small rows ew ew_blocks rps kind")


def ceil_div(a, b):
    return -(-a // b)


def dispatch32(shape, layouts=("plain",)):
    """The variant the fp32 entries take for operands of `shape` in `layouts` (one per operand: any operand can take the vector path away)"""
    N, C, D, H, W = five(shape)
    hw = H * W
    contig, v4 = True, hw % 4 == 0
    for lay in layouts:
        (sn, sc, sd, sh, sw), off, _ = layout_of(shape, lay)
        if D == 1:
            sd = 0
        contig = contig and (W == 1 or sw == 1) and (H == 1 or sh == W)
        v4 = v4 and sn % 4 == 0 and sc % 4 == 0 and sd % 4 == 0 and off % 4 == 0      # GUARD and the allocator keep the storage itself 16-byte aligned
    v4 = v4 and contig
    inner, vec = (hw if contig else 1), (4 if v4 else 1)
    gpr = hw // vec if contig else hw
    groups, per_chan = N * C * D * gpr, N * D * gpr
    split = max(1, min(ceil_div(2048, C), ceil_div(per_chan, 1024)))
    seg = ceil_div(per_chan, split)
    small = vec == 4 and inner != 1 and 64 <= per_chan <= 8192 and C >= 32 and groups < (1 << 28)
    rows = vec == 4 and inner != 1 and gpr % 256 == 0
    ew = "ew_rows" if rows else "ew<4>" if vec == 4 else "ew<1>"
    kind = "small" if small else "rows" if rows else "gen4" if vec == 4 else "gen1"
    return Dispatch(vec, inner, gpr, groups, per_chan, split, seg, small, rows, ew, min(max(ceil_div(groups, 256), 1), 8192), ceil_div(N * D, split), kind)


def note_forward(d, training=True):
    if not training:
        return f"bn_eval_stats_kernel + BnApply {d.ew}"
    if d.small:
        return f"bn_fwd_small_kernel ({d.per_chan} groups per channel, one launch)"
    return f"bn_stats_kernel<{d.vec}> x {d.split} blocks per channel + bn_finalize_kernel + BnApply {d.ew}"


def note_backward(d):
    if d.small:
        return f"bn_bwd_small_kernel ({d.per_chan} groups per channel, one launch)"
    red = "bn_bwd_reduce_rows_kernel" if d.rows else f"bn_bwd_reduce_kernel<{d.vec}>"
    return f"{red} x {d.split} blocks per channel + bn_bwd_finalize_kernel + BnBwdApply {d.ew}"


def note_forward_stats(d, nparts, pitch):
    if d.small:
        return f"bn_fwd_small_kernel ({d.per_chan} groups per channel, one launch; the {nparts} partials are not read)"
    return f"bn_partials_finalize_kernel ({nparts} partials, pitch {pitch}) + BnApply {d.ew}"


def note_sync_sums(d):
    return f"bn_stats_kernel<{d.vec}> x {d.split} blocks per channel + bn_sync_fold_kernel (rank row)"


def note_sync_backward_sums(d):
    red = "bn_bwd_reduce_rows_kernel" if d.rows else f"bn_bwd_reduce_kernel<{d.vec}>"
    return f"{red} x {d.split} blocks per channel + bn_sync_fold_kernel (rank row)"


# ... and of csrc/cl_elementwise.hip (cl_bn_setup, cl_bn_block_out)
DispatchCL = namedtuple("DispatchCL", "G pb blocks P combine active per_thread")


def dispatch_cl(shape):
    N, C, D, H, W = five(shape)
    assert C % 8 == 0 and C <= 1024
    G, P = C // 8, N * D * H * W
    pb = max(1, 256 // G)
    blocks = min(max(ceil_div(P, 8 * pb), 1), 1024)
    combine = "xor" if (G & (G - 1)) == 0 and G <= 64 else "serial"
    return DispatchCL(G, pb, blocks, P, combine, pb * G, ceil_div(P, blocks * pb))


def note_cl(d, what):
    if what == "eval":
        return f"cl_bn_coeff_kernel (running statistics) + cl_bn_apply_kernel: G {d.G}, pb {d.pb}"
    passes = {"forward": "cl_bn_stats_kernel + cl_bn_finalize_kernel + cl_bn_apply_kernel",
              "backward": "cl_bn_bwd_reduce_kernel + cl_bn_bwd_finalize_kernel + cl_bn_bwd_apply_kernel"}[what]
    return f"{passes}: G {d.G}, pb {d.pb}, blocks {d.blocks}, {d.combine} combine"


def note_cl_stats(d, nparts, pitch):
    return f"cl_bn_finalize_stat_kernel ({nparts} partials, pitch {pitch}) + cl_bn_apply_kernel: G {d.G}, pb {d.pb}"


# ------------------------------------------------------------------------------------------------------------------------------------------------------
# the case tables.  want: the variant the case is meant to hit — kind, split, and properties of the segmentation (test_bn_exact_cpu.py checks the
# arithmetic above against them; the GPU tests assert the device's note)
# ------------------------------------------------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "name shape layout want")

CASES32 = [
    Case("small_min", (4, 32, 8, 8), "plain", dict(kind="small", per_chan=64)),
    Case("below_small", (7, 32, 6, 6), "plain", dict(kind="gen4", split=1, per_chan=63)),
    Case("small_max", (8, 32, 64, 64), "plain", dict(kind="small", per_chan=8192)),
    Case("small_ragged_a", (5, 48, 3, 28, 28), "plain", dict(kind="small", ragged_slot=True)),
    Case("small_ragged_b", (3, 40, 5, 12, 12), "plain", dict(kind="small", ragged_slot=True)),
    Case("above_small", (9, 32, 64, 64), "plain", dict(kind="rows", split=9, rps=1, per_chan=9216)),
    Case("rows_empty_blocks", (7, 5, 48, 64), "plain", dict(kind="rows", split=6, rps=2, gpr=768, empty_blocks=2)),
    Case("rows_3d", (2, 3, 5, 32, 32), "plain", dict(kind="rows", split=3, rps=4)),
    Case("gen4_split_a", (6, 3, 5, 20, 20), "plain", dict(kind="gen4", split=3, seg_spans_rows=True)),
    Case("gen4_split_b", (11, 3, 2, 22, 22), "plain", dict(kind="gen4", split=3, clamped=True)),
    Case("gen1_odd_a", (3, 33, 7, 9), "plain", dict(kind="gen1", split=1)),
    Case("gen1_odd_b", (5, 2, 3, 15, 15), "plain", dict(kind="gen1", split=4, clamped=True)),
    Case("gen1_misaligned", (4, 6, 8, 8), "misaligned", dict(kind="gen1", inner=64)),
    Case("gen1_stride", (3, 4, 8, 8), "nstride2", dict(kind="gen1", inner=64)),
    Case("inner1_step", (3, 5, 6, 8), "wstep2", dict(kind="gen1", inner=1)),
    Case("inner1_transposed", (3, 5, 6, 8), "hw_transposed", dict(kind="gen1", inner=1)),
    Case("permuted_rows", (2, 3, 5, 32, 32), "permuted", dict(kind="rows", split=3)),
    Case("permuted_small", (4, 32, 2, 8, 8), "permuted", dict(kind="small")),
    Case("slice_small", (5, 48, 3, 28, 28), ("slice", 64, 8), dict(kind="small")),
    Case("slice_rows", (2, 3, 5, 32, 32), ("slice", 7, 2), dict(kind="rows", split=3)),
    Case("stride_vec1", (4, 6, 9, 99, 99), "plain", dict(kind="gen1", split=342, groups=2117016, grid_stride=True)),
    Case("stride_vec4", (6, 6, 10, 140, 172), "plain", dict(kind="gen4", groups=2167200, grid_stride=True)),
]
TANH_CASES = ["small_ragged_a", "rows_3d"]

CASES_CL = (
    [Case(f"xor_c{c}", (5, c, 9, 11), "plain", dict(combine="xor")) for c in (8, 16, 32, 64, 128, 256, 512)]
    + [Case(f"xor_pow2_c{c}", (4, c, 8, 8), "plain", dict(combine="xor", count_pow2=True)) for c in (8, 16, 32, 64, 128, 256, 512)]
    + [Case(f"serial_c{c}", (4, c, 6, 10), "plain", dict(combine="serial", active=a)) for c, a in ((24, 255), (40, 255), (96, 252), (192, 240), (384, 240), (768, 192))]
    + [Case("g128", (3, 1024, 5, 7), "plain", dict(combine="serial", G=128, lds_bytes=65536)),
       Case("pix3d_xor", (2, 32, 5, 6, 6), "plain", dict(combine="xor")),
       Case("pix3d_serial", (3, 96, 4, 3, 5), "plain", dict(combine="serial")),
       Case("few_pixels", (3, 128, 1, 1), "plain", dict(combine="xor", idle_slots=True)),
       Case("block_cap", (5, 768, 41, 80), "plain", dict(combine="serial", blocks=1024, per_thread=9)),
       Case("slice_xor", (4, 64, 8, 8), ("slice", 96, 16), dict(combine="xor")),
       Case("slice_serial", (4, 96, 6, 10), ("slice", 128, 8), dict(combine="serial"))]
)


def by_name(table, name):
    return next(c for c in table if c.name == name)


# ------------------------------------------------------------------------------------------------------------------------------------------------------
# operands
# ------------------------------------------------------------------------------------------------------------------------------------------------------
Operands = namedtuple("Operands", "x dy gamma beta mask m a rm rv")


def per_channel(v, ndim):
    return v.view(1, -1, *([1] * (ndim - 2)))


def exact_operands(name, shape):
    """fp64 operands of the integer scheme, in logical (N, C, ...) order.  rm / rv: the eval-mode running statistics (an integer, and 1/4, 1 or 4)."""
    g = torch.Generator().manual_seed(seed_of(name))
    N, C = shape[0], shape[1]
    sp = tuple(shape[2:])
    per = N * math.prod(sp)
    m = torch.randint(-8, 9, (C,), generator=g).double()
    a = (2.0 ** torch.randint(0, 3, (C,), generator=g)).double()
    rank = torch.rand(C, per, generator=g).argsort(1)                      # a seeded random half of the positions of every channel gets +
    sign = torch.where(rank < per // 2, 1.0, -1.0).double()                # (odd count: one - more: the balance cannot hold there)
    sign = sign.view((C, N) + sp).transpose(0, 1).contiguous()
    x = per_channel(m, len(shape)) + sign * per_channel(a, len(shape))
    dy = torch.randint(-4, 5, tuple(shape), generator=g).double()
    gamma = (2.0 ** torch.randint(-1, 2, (C,), generator=g)).double()
    beta = torch.randint(-3, 4, (C,), generator=g).double()
    mask = (torch.rand(N, C, generator=g) < 0.5).double() * 2.0
    rm = m + torch.randint(-1, 2, (C,), generator=g).double()
    rv = (4.0 ** torch.randint(-1, 2, (C,), generator=g)).double()
    return Operands(x, dy, gamma, beta, mask, m, a, rm, rv)


def real_operands(name, shape, bf16=False, eps=1e-5, margin=1e-4):
    """N(0.4, 1.7^2) inputs (bf16 values for the channels-last path), moved off LeakyReLU's kink the way tests/test_sync_bn_gpu.py::off_the_kink does"""
    g = torch.Generator().manual_seed(seed_of("real:" + name))
    N, C = shape[0], shape[1]
    rnd = (lambda t: t.bfloat16().float()) if bf16 else (lambda t: t)
    x = rnd(torch.randn(tuple(shape), generator=g) * 1.7 + 0.4)
    gamma = torch.rand(C, generator=g) + 0.5
    beta = torch.randn(C, generator=g)
    dy = rnd(torch.randn(tuple(shape), generator=g))
    mask = (torch.rand(N, C, generator=g) < 0.5).float() * 2.0
    rm, rv = torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) + 0.5
    for _ in range(6):
        z = torch.nn.functional.batch_norm(x.double(), None, None, gamma.double(), beta.double(), True, 0.0, eps)
        near = z.abs() < margin
        if not bool(near.any()):
            break
        x = torch.where(near, rnd(x + (0.0625 if bf16 else 0.01)), x)
    else:
        raise AssertionError("could not move the test input off the activation's kink")
    return Operands(x.double(), dy.double(), gamma.double(), beta.double(), mask.double(), None, None, rm.double(), rv.double())


# ------------------------------------------------------------------------------------------------------------------------------------------------------
# the fp64 reference: plain formulas (test_bn_exact_cpu.py checks them against F.batch_norm in fp64 plus autograd)
# ------------------------------------------------------------------------------------------------------------------------------------------------------
Ref = namedtuple("Ref", "count s0 s1 mean var invstd y dz xh sdz sdzx k0 k1 dx dgamma dbeta rm rv")


def act_of(mode):
    """-> (uses the dropout mask, activation name)"""
    return mode == "dropout", {"leaky": "leaky", "dropout": "leaky", "none": "none", "eval": "leaky", "tanh": "tanh"}[mode]


def reference(o, mode, eps=0.0, momentum=0.5, mean=None, invstd=None, slope=SLOPE, rm0=None, rv0=None):
    """Everything the kernels produce, in fp64.  mode "eval" normalises with o.rm / o.rv; `mean` / `invstd` (per channel) replace the batch statistics in the
    normalisation and the backward pass (the backward entry takes them as arguments)."""
    x, nd = o.x, o.x.dim()
    dims = (0,) + tuple(range(2, nd))
    count = x.numel() // x.shape[1]
    s0, s1 = x.sum(dims), (x * x).sum(dims)
    bmean = s0 / count
    bvar = (s1 / count - bmean * bmean).clamp_min(0.0)
    training = mode != "eval"
    if mean is None:
        mean, invstd = (bmean, 1.0 / torch.sqrt(bvar + eps)) if training else (o.rm, 1.0 / torch.sqrt(o.rv + eps))
    use_mask, act = act_of(mode)
    mk = o.mask.view(o.mask.shape + (1,) * (nd - 2)) if use_mask else torch.ones((), dtype=torch.float64)
    pc = lambda v: per_channel(v, nd)
    xh = (x - pc(mean)) * pc(invstd)
    z = (xh * pc(o.gamma) + pc(o.beta)) * mk
    if act == "leaky":
        y, dact = torch.where(z > 0, z, z * slope), torch.where(z > 0, torch.ones_like(z), torch.full_like(z, slope))
    elif act == "tanh":
        y = torch.tanh(z); dact = 1.0 - y * y
    else:
        y, dact = z, torch.ones_like(z)
    dz = o.dy * mk * dact
    sdz, sdzx = dz.sum(dims), (dz * xh).sum(dims)
    k0, k1 = (sdz / count, sdzx / count) if training else (torch.zeros_like(sdz), torch.zeros_like(sdz))
    dx = pc(o.gamma * invstd) * (dz - pc(k0) - xh * pc(k1))
    rm0 = torch.zeros_like(mean) if rm0 is None else rm0
    rv0 = torch.ones_like(mean) if rv0 is None else rv0
    unb = bvar * count / (count - 1) if count > 1 else bvar
    rm, rv = (1 - momentum) * rm0 + momentum * bmean, (1 - momentum) * rv0 + momentum * unb
    return Ref(count, s0, s1, mean, bvar, invstd, y, dz, xh, sdz, sdzx, k0, k1, dx, sdzx, sdz, rm, rv)


# ------------------------------------------------------------------------------------------------------------------------------------------------------
# what is exact, and the rounding bounds of what is not
# ------------------------------------------------------------------------------------------------------------------------------------------------------
def is_f32(t):
    return t.float().double() == t


def is_bf16(t):
    return (t.bfloat16().double() == t) & (t.abs() <= 256)


def sums_exact(o, r, run, mode):
    """The raw sums: integers (multiples of 1/8 in the backward pass), every fp32 run of `run` terms below 2^24 in units of the operands' grid — so ANY order of
    adding them is exact, in fp32 inside a run and in fp64 across runs.  Raises if the construction does not deliver that."""
    assert bool((o.x == o.x.round()).all()) and float(o.x.abs().max()) ** 2 * run < 2 ** 24
    assert bool((r.s0 == r.s0.round()).all()) and bool((r.s1 == r.s1.round()).all())
    g = 8.0          # dz is a multiple of 1/4; xhat is +-1 in training and a multiple of 1/2 in eval mode ((x - rm) / sqrt(rv))
    assert bool(((r.dz * r.xh * g) == (r.dz * r.xh * g).round()).all()) and float((r.dz * r.xh).abs().max()) * g * run < 2 ** 24
    assert bool(is_f32(r.sdz).all()) and bool(is_f32(r.sdzx).all()), "dbeta / dgamma are not fp32 values"
    return True


def stats_exact(o, r):
    """Per case: mean = m and var = a^2 exactly (needs the +- balance: an even count)"""
    return bool((r.mean == o.m).all()) and bool((r.var == o.a * o.a).all())


def y_exact(o, r):
    """Per element: x sc, sh and y are fp32 values, so the apply pass is exact whether or not the compiler fuses the multiply-add"""
    nd = o.x.dim()
    sc = o.gamma * r.invstd
    sh = o.beta - r.mean * sc
    ok = is_f32(sc) & is_f32(sh) & is_f32(r.mean) & is_f32(r.invstd) & is_f32(r.mean * sc)
    return per_channel(ok, nd) & is_f32(o.x * per_channel(sc, nd)) & is_f32(r.y)


def dx_exact(o, r):
    """Per element: every intermediate of ga is (dz - k0 - xhat k1) is an fp32 value (count a power of two and short significands in the sums give that)"""
    nd = o.x.dim()
    pc = lambda v: per_channel(v, nd)
    ok = is_f32(r.k0) & is_f32(r.k1) & is_f32(o.gamma * r.invstd) & is_f32(r.mean) & is_f32(r.invstd)
    t1, t2 = r.dz - pc(r.k0), r.xh * pc(r.k1)
    return pc(ok) & is_f32(r.xh) & is_f32(r.dz) & is_f32(t1) & is_f32(t2) & is_f32(t1 - t2) & is_f32(r.dx)


def dx_bound(o, r, roundings=4, run=0, ddz=None):
    """|dx - dx_ref| where dx is not exact, by counting roundings.  The device evaluates ga is (dz - k0 - xhat k1) with k0 = fl(sum dz / count) and
    k1 = fl(sum dz xhat / count): one rounding each (the sums and the fp64 division carry 2^-53).  In the integer scheme xhat = +-1 (or a multiple of 1/2), dz and
    ga is are exact, so the roundings left are: k0 (1), k1 (1), fl(dz - k0) (1), fl(xhat k1) (0: a power-of-two multiple), the second subtraction (1), the product
    with the power of two ga is (0).  No summand passes through more than 4 of them (k0: its own, two subtractions; k1: its own, one subtraction; dz: two
    subtractions), each rounding is at most U = 2^-24 relative to a partial result no larger than |dz| + |k0| + |xhat k1|, hence
        |dx - dx_ref| <= 4 U |ga is| (|dz| + |k0| + |xhat k1|).
    Real-valued operands (`roundings` = 8): xhat = fl(fl(x - mu) is) adds 2, fl(xhat k1) 1 and fl(ga is) 1 to the k1 summand's 3 + the final product = 8; and the
    fp32 runs of `run` terms in the two sums move k0 by run U mean|dz| and k1 by (run + 3) U mean|dz xhat| (recursive summation, n u; 3 for the roundings inside
    each term dz xhat).  `ddz`: an elementwise error of dz itself (the Tanh branch), which enters directly and through both means."""
    nd = o.x.dim()
    pc = lambda v: per_channel(v, nd)
    dims = (0,) + tuple(range(2, nd))
    gi = pc((o.gamma * r.invstd).abs())
    b = roundings * U * gi * (r.dz.abs() + pc(r.k0.abs()) + (r.xh * pc(r.k1)).abs())
    if run:
        b = b + gi * (run * U * pc(r.dz.abs().mean(dims)) + r.xh.abs() * (run + 3) * U * pc((r.dz * r.xh).abs().mean(dims)))
    if ddz is not None:
        b = b + gi * (ddz + pc(ddz.mean(dims)) + r.xh.abs() * pc((ddz * r.xh.abs()).mean(dims)))
    return b


def cl_coefficients(o, r, training=True):
    """cl_bn_bwd_finalize_kernel's coefficients in fp64: dx = k1 dz - k2 - k3 x"""
    k1 = o.gamma * r.invstd
    if not training:
        return k1, torch.zeros_like(k1), torch.zeros_like(k1)
    k3 = k1 * r.invstd * r.k1
    return k1, k1 * r.k0 - k3 * r.mean, k3


def cl_dx_exact(o, r, training=True):
    """The channels-last backward apply evaluates k1 dz - k2 - k3 x with k1, k2, k3 rounded to fp32 from fp64: exact where they and every intermediate are fp32
    values.  (The result is then rounded to 16 bits once, to nearest even: the expected output is that rounding of the reference.)"""
    nd = o.x.dim()
    pc = lambda v: per_channel(v, nd)
    k1, k2, k3 = cl_coefficients(o, r, training)
    ok = is_f32(k1) & is_f32(k2) & is_f32(k3) & is_f32(r.mean) & is_f32(r.invstd)
    t1, t2 = pc(k1) * r.dz, pc(k3) * o.x
    return pc(ok) & is_f32(r.dz) & is_f32(t1) & is_f32(t1 - pc(k2)) & is_f32(t2) & is_f32(t1 - pc(k2) - t2) & (t1 - pc(k2) - t2 == r.dx)


def cl_dx_bound(o, r, roundings=4, run=0, training=True):
    """As dx_bound for k1 dz - k2 - k3 x: k2 and k3 round once each on the way to fp32, the two products and the two subtractions once each; no summand passes
    through more than 4 (k3 x: k3, product, second subtraction; k2: its own, both subtractions; k1 dz: product, both subtractions) with k1 exact in the integer
    scheme; real-valued operands add fl(dy mask), the slope and k1's own rounding (`roundings` = 7).  Each is U relative to a partial result no larger than
    |k1 dz| + |k2| + |k3 x| — the summands, not the result: k2 and k3 x nearly cancel.  `run`: the sums' fp32 runs move k2 and k3 (see dx_bound)."""
    nd = o.x.dim()
    pc = lambda v: per_channel(v, nd)
    dims = (0,) + tuple(range(2, nd))
    k1, k2, k3 = cl_coefficients(o, r, training)
    b = roundings * U * ((pc(k1) * r.dz).abs() + pc(k2.abs()) + (pc(k3) * o.x).abs())
    if run and training:
        e0, e1 = run * U * r.dz.abs().mean(dims), (run + 3) * U * (r.dz * r.xh).abs().mean(dims)
        dk3 = (k1 * r.invstd).abs() * e1
        b = b + pc(k1.abs() * e0 + dk3 * r.mean.abs()) + pc(dk3) * o.x.abs()
    return b


def y_bound(o, r, dmean=None, dis_rel=None, roundings=6):
    """|y - y_ref| before the activation's power-of-two (or <= 1) factor.  The device forms sc = fl(ga is), sh = fl(be - fl(mu sc)), z = fl(fl(x sc) + sh), times
    the mask (a power of two: exact) and, for LeakyReLU 0.2, one more product.  Roundings per summand: x sc: sc, product, sum, slope = 4; mu sc: sc, product, sh, sum,
    slope = 5 (the channels-last finalize forms fl(fl(fl(mu) ga) is) instead: 6); be: sh, sum, slope = 3 — at most 6, each U relative to a partial result no larger
    than |x sc| + |mu sc| + |be|.  A statistics error (`dmean` absolute, `dis_rel` relative in invstd, per channel) moves z by |sc| dmean + |(x - mu) sc| dis_rel."""
    nd = o.x.dim()
    pc = lambda v: per_channel(v, nd)
    sc = o.gamma * r.invstd
    b = roundings * U * ((o.x * pc(sc)).abs() + pc((r.mean * sc).abs()) + pc(o.beta.abs()))
    if dmean is not None:
        b = b + pc(sc.abs() * dmean) + ((o.x - pc(r.mean)) * pc(sc)).abs() * pc(dis_rel)
    return b


def stat_bounds(o, r, run, eps):
    """The statistics of real-valued input: n u bound of recursive summation over fp32 runs of `run` terms (the fp64 part carries 2^-53).
    -> (bound on |mean - mean64|, bound on |var - var64|, and for the apply pass's bound: dmean incl. the fp32 rounding of save_mean, the relative error of invstd, and the
    whole error of var = E x^2 - mean^2)"""
    nd = o.x.dim()
    dims = (0,) + tuple(range(2, nd))
    bm = run * U * o.x.abs().mean(dims)
    bv = run * U * (o.x * o.x).mean(dims)
    dvar = bv + 2 * r.mean.abs() * bm + bm * bm                   # var = E x^2 - mean^2: the mean's error enters as well
    dis = 1.0 / torch.sqrt(1.0 - dvar / (r.var + eps)) - 1.0 + 2 * U      # worst case of (var + eps - dvar)^-1/2, plus the fp32 rounding of invstd
    return bm, bv, bm + U * r.mean.abs(), dis, dvar


def ulp32(t):
    """Spacing of fp32 at |t| (t: fp64)"""
    f = t.float().abs().clamp_min(2.0 ** -126)
    return (torch.nextafter(f, torch.full_like(f, float("inf"))) - f).double()


# ------------------------------------------------------------------------------------------------------------------------------------------------------
# comparison and the mismatch report
# ------------------------------------------------------------------------------------------------------------------------------------------------------
def owner32(d, shape, idx):
    """Which block / segment / slot / row of the fp32 dispatch owns element idx = (n, c, d, h, w)"""
    N, C, D, H, W = five(shape)
    n, c, dd, h, w = idx
    g = (n * D + dd) * d.gpr + (h * W + w) // (d.vec if d.inner != 1 else 1)
    if d.small:
        return f"small kernel: channel block {c}, slot {g // 1024}, thread {g % 1024}"
    s = g // d.seg
    gg = ((n * C + c) * D + dd) * d.gpr + (h * W + w) // (d.vec if d.inner != 1 else 1)
    red = f"statistics / generic reduce: segment {s} of {d.split} (block {c * d.split + s}), thread {(g - s * d.seg) % 256}, trip {(g - s * d.seg) // 256}"
    if d.rows:
        row = n * D + dd
        return f"{red}; rows reduce: row {row}, block {c * d.split + row // d.rps}; ew_rows: block {(n * C + c) * D + dd}, thread {(h * W + w) // 4 % 256}"
    return f"{red}; {d.ew}: group {gg}, block {gg // 256 % d.ew_blocks}, grid-stride trip {gg // (256 * d.ew_blocks)}"


def owner_cl(d, shape, idx):
    N, C, D, H, W = five(shape)
    n, c, dd, h, w = idx
    q = n * D * H * W + (dd * H + h) * W + w
    return (f"pixel {q}: reduce block {q // d.pb % d.blocks}, slot {q % d.pb}, group {c // 8} (thread {q % d.pb * d.G + c // 8}), "
            f"trip {q // (d.pb * d.blocks)}; {d.combine} combine")


def first_mismatch(bad, got, want, shape, owner):
    """A description of the first element where `bad` holds"""
    flat = int(bad.reshape(-1).nonzero()[0])
    idx5 = tuple(int(v) for v in torch.unravel_index(torch.tensor(flat), five(shape))) if got.dim() > 1 else (0, flat, 0, 0, 0)
    gv, wv = float(got.reshape(-1)[flat]), float(want.reshape(-1)[flat])
    where = owner(idx5) if (owner is not None and got.dim() > 1) else ""
    return f"{int(bad.sum())} of {bad.numel()} elements differ; first at (n, c, d, h, w) = {idx5}: got {gv!r}, expected {wv!r}, difference {gv - wv!r}.  {where}"


def assert_within(what, got, want, bound, shape, owner=None, bf16=False):
    """got (device result on the host, any float type) against the fp64 `want`: |got - want| <= bound elementwise, bit-equal where bound is 0.  bf16 results must
    lie between the bf16 roundings of want - bound and want + bound (equal to the rounding of want where bound is 0).  -> worst error / bound over the elements
    with a non-zero bound."""
    got = got.detach().cpu()
    bound = torch.as_tensor(bound, dtype=torch.float64).expand_as(want)
    g = got.double()
    if bf16:
        bad = ~((g >= (want - bound).bfloat16().double()) & (g <= (want + bound).bfloat16().double()))
    else:
        bad = ~((g - want).abs() <= bound)
    if bool(bad.any()):
        raise AssertionError(f"{what}: " + first_mismatch(bad, g, want, shape, owner))
    nz = bound > 0
    if bf16 or not bool(nz.any()):
        return 0.0
    return float(((g - want).abs()[nz] / bound[nz]).max())
