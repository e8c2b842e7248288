"""Host side of the exact elementwise / RNG / loss / GRU / channel-softmax / flow checks (tests/test_ew_exact_cpu.py, tests/test_ew_exact_gpu.py).  No GPU is
touched here.

Every expected value of those tests is made here from the operands alone: in fp64, or in fp32 numpy where the kernel's operation order is reproducible (the
Philox words and their fp32 uniforms, the __fadd_rn / __fmul_rn chain of the uint8 conversion).  Operands are chosen so that what can be exact is exact (small
integers, power-of-two factors, tanh outputs on a 1/8 grid, logits on a 2^-10 grid), and `*_exact` / `*_bound` decide FROM THE OPERANDS AND THE REFERENCE ALONE
which results must match bit for bit and how far the others may be off, by counting roundings.  The layouts, guard bands and the dispatch arithmetic come from
tests/exactbn.py; Philox4x32-10 and its fp32 uniform from tests/test_augment_cpu.py (checked there against the published vectors)."""
import math
from collections import namedtuple

import numpy as np
import torch

from tests import exactbn as X
from tests.test_augment_cpu import philox4x32_10, u01

F32, F64, U32 = np.float32, np.float64, np.uint32
U = X.U                           # fp32 unit roundoff, 2^-24; one ulp is at most 2 U relative
TINY = 2.0 ** -126                # smallest normal fp32: below it a result may be flushed to zero, an absolute error of less than TINY
SLOPE = 0.25
AXPBY_A, AXPBY_B = 0.5, -2.0
# OpenCL C specification, "Relative error as ULPs" (the source tests/test_bn_exact_gpu.py names for TANH_ULPS): exp <= 3 ulp, log1p <= 2 ulp, x / y <= 2.5 ulp
EXP_ULPS, LOG1P_ULPS, DIV_ULPS = 3, 2, 2.5
NORMAL_CAP = 2.0 ** -10           # |z - z_ref| <= NORMAL_CAP (1 + |z_ref|): a cap, not a measurement (__logf / __sincosf carry no specified accuracy)
NORMAL_FINDING = 2.0 ** -14       # an observed error above this is reported, the cap stays
SEED_HI, OFFSET_HI = 0x123456789ABCDEF0, 2 ** 33 + 5      # all four counter words and both key words non-zero
RNG_N = (1, 3, 4, 5, 1023, 1024, 1025, 131073)
DROPOUT_EXACT_P, DROPOUT_ULP_P = (0.0, 0.5, 0.75), (0.25, 0.9)


# ------------------------------------------------------------------------------------------------------------------------------------------------------
# 1. the fp32 elementwise dispatcher: cases, operands, expectations
# ------------------------------------------------------------------------------------------------------------------------------------------------------
EwCase = namedtuple("EwCase", "name shape combos path big")
# combo: a layout for every operand, or ("first", L) / ("last", L): L on the first / last operand and plain on the others
EW_CASES = [
    EwCase("rows_1024", (2, 3, 2, 32, 32), ["plain"], "ew_rows", False),
    EwCase("rows_2048", (1, 2, 1, 32, 64), ["plain", ("slice", 5, 2)], "ew_rows", False),
    EwCase("gen4", (2, 3, 6, 8, 8), ["plain", "permuted", ("slice", 7, 3)], "ew<4>", False),
    EwCase("lost_vec", (2, 3, 6, 8, 8), [("first", "misaligned"), ("last", "misaligned"), ("first", "nstride2"), ("last", "nstride2")], "ew<1> inner!=1", False),
    EwCase("odd_plane", (3, 5, 2, 7, 9), ["plain", "permuted"], "ew<1> inner!=1", False),
    EwCase("scattered", (2, 3, 2, 6, 10), ["wstep2", "hw_transposed", ("first", "wstep2"), ("last", "hw_transposed")], "ew<1> inner=1", False),
    EwCase("degenerate_nc", (4, 7, 1, 1), ["plain"], "ew<1> inner=1", False),
    EwCase("degenerate_w", (1, 1, 1, 1, 5), ["plain"], "ew<1> inner!=1", False),
    EwCase("degenerate_d", (3, 1, 4, 1, 1), ["plain"], "ew<1> inner=1", False),
    EwCase("stride_tail", (2, 1, 1, 1025, 1025), ["plain"], "ew<1> inner!=1", True),      # act_forward and noise_add only: 8 MB per operand
]
EW_PATHS = {"ew_rows", "ew<4>", "ew<1> inner!=1", "ew<1> inner=1"}
EW_PARAMS = [(c.name, i) for c in EW_CASES for i in range(len(c.combos))]


def ew_case(name):
    return X.by_name(EW_CASES, name)


def operand_layouts(combo, k):
    """The layouts of an entry's k operands (inputs first, the output last) under `combo`"""
    if isinstance(combo, tuple) and combo[0] in ("first", "last"):
        lays = ["plain"] * k
        lays[0 if combo[0] == "first" else k - 1] = combo[1]
        return tuple(lays)
    return (combo,) * k


def ew_path(shape, layouts):
    """-> (the kernel launch_ew takes, as one of EW_PATHS; the Dispatch)"""
    d = X.dispatch32(shape, tuple(layouts))
    return (d.ew if d.ew != "ew<1>" else "ew<1> inner=1" if d.inner == 1 else "ew<1> inner!=1"), d


def ew_operands(name, shape):
    """x, z, dy: integers in [-64, 64] (x with zeros, LeakyReLU's kink); yt: tanh outputs k / 8, |k| <= 7; yl: LeakyReLU outputs (integers); all fp64, logical order"""
    g = torch.Generator().manual_seed(X.seed_of("ew:" + name))
    r = lambda lo, hi: torch.randint(lo, hi + 1, tuple(shape), generator=g).double()
    return dict(x=r(-64, 64), z=r(-64, 64), dy=r(-64, 64), yl=r(-64, 64), yt=r(-7, 7) / 8.0)


def act_forward_ref(x, act, slope=SLOPE):
    return {"none": x, "leaky": torch.where(x > 0, x, x * slope), "tanh": torch.tanh(x)}[act]


def act_backward_ref(dy, y, act, slope=SLOPE):
    return dy * {"none": torch.ones_like(y), "leaky": torch.where(y > 0, torch.ones_like(y), torch.full_like(y, slope)), "tanh": 1.0 - y * y}[act]


def axpby_ref(x, z=None, a=AXPBY_A, b=AXPBY_B):
    return a * x if z is None else a * x + b * z


def ew_exactness(o):
    """Every intermediate and result of the exact expectations is an fp32 value, so the order of rounding and contraction cannot matter.  -> True, or raises"""
    f = lambda t: bool(X.is_f32(t).all())
    assert f(o["x"] * SLOPE) and f(act_forward_ref(o["x"], "leaky"))
    assert f(o["yt"] * o["yt"]) and f(1.0 - o["yt"] * o["yt"]) and f(act_backward_ref(o["dy"], o["yt"], "tanh"))
    assert f(act_backward_ref(o["dy"], o["yl"], "leaky"))
    assert f(AXPBY_A * o["x"]) and f(AXPBY_B * o["z"]) and f(axpby_ref(o["x"], o["z"]))
    assert float(o["x"].abs().max()) <= 64 and float(o["dy"].abs().max()) <= 64 and float((o["yt"] * 8).abs().max()) <= 7
    assert bool((o["yt"] * 8 == (o["yt"] * 8).round()).all())
    return True


def u8_operands(name, shape):
    """fp32 in [-1.5, 1.5] with the clip's and the truncation's edges planted at the front"""
    g = torch.Generator().manual_seed(X.seed_of("u8:" + name))
    x = (torch.rand(tuple(shape), generator=g) * 3.0 - 1.5).float().numpy()
    one = F32(1.0)
    edge = np.array([1.0, -1.0, 0.0, -0.0, np.nextafter(one, F32(2)), np.nextafter(one, F32(0)), np.nextafter(-one, F32(-2)), np.nextafter(-one, F32(0)), 1.5, -1.5], dtype=F32)
    flat = x.reshape(-1)
    n = min(flat.size, edge.size)
    flat[:n] = edge[:n]
    return flat.reshape(tuple(shape))


def to_u8_ref(x, rep):
    """uint8(int(((clip(x, -1, 1) + 1) * 0.5) * 255)), every step rounded to fp32 (the kernel's __fadd_rn / __fmul_rn chain); out (N, C rep, ...): channel c rep + q"""
    x = np.asarray(x, dtype=F32)
    t = np.clip(x, F32(-1), F32(1))
    t = ((t + F32(1)).astype(F32) * F32(0.5)).astype(F32) * F32(255)
    b = t.astype(F32).astype(np.int32).astype(np.uint8)
    return np.repeat(b, rep, axis=1)


# ------------------------------------------------------------------------------------------------------------------------------------------------------
# 2. the RNG contract: key = seed, counter {q lo, q hi, offset lo, offset hi}, q = element // 4; Box-Muller pairs
# ------------------------------------------------------------------------------------------------------------------------------------------------------
M32 = 0xFFFFFFFF


def philox_words(nq, seed, offset, q0=0):
    """-> (nq, 4) uint32: the words of counters q0 .. q0 + nq - 1 of the stream (seed, offset)"""
    q = np.arange(q0, q0 + nq, dtype=np.uint64)
    ctr = np.stack([q & np.uint64(M32), q >> np.uint64(32), np.full_like(q, offset & M32), np.full_like(q, (offset >> 32) & M32)], 1)
    return philox4x32_10(ctr, (seed & M32, (seed >> 32) & M32))


def dropout_ref(n, p, seed, offset):
    """mask[i] = keep if u01(word[i % 4] of counter i // 4) >= p else 0, all in fp32; keep = 1 / (1 - p) in fp32"""
    u = u01(philox_words((n + 3) // 4, seed, offset)).reshape(-1)[:n]
    keep = F32(1) / (F32(1) - F32(p))
    return np.where(u >= F32(p), keep, F32(0)).astype(F32)


def normals_of_words(words):
    """(nq, 4) words -> (nq, 4) fp64 normals (r0 cos, r0 sin, r1 cos, r1 sin): r = sqrt(-2 ln max(u, 1e-30)) of the fp32 uniform, angle = the fp32 product
    6.2831855f * u taken to fp64"""
    u = u01(words)
    assert u.dtype == F32
    r0 = np.sqrt(-2.0 * np.log(np.maximum(u[:, 0], F32(1e-30)).astype(F64)))
    r1 = np.sqrt(-2.0 * np.log(np.maximum(u[:, 2], F32(1e-30)).astype(F64)))
    a0 = (F32(6.283185307179586) * u[:, 1]).astype(F32).astype(F64)
    a1 = (F32(6.283185307179586) * u[:, 3]).astype(F32).astype(F64)
    return np.stack([r0 * np.cos(a0), r0 * np.sin(a0), r1 * np.cos(a1), r1 * np.sin(a1)], 1)


def normal_ref(n, seed, offset):
    return normals_of_words(philox_words((n + 3) // 4, seed, offset)).reshape(-1)[:n]


def normal_many_ref(n, count, seed, offset):
    """draw j is normal_ref(n, seed, offset + j)"""
    return np.stack([normal_ref(n, seed, offset + j) for j in range(count)], 0)


def normal_err(z, ref):
    """-> max |z - ref| / (1 + |ref|)"""
    z, ref = np.asarray(z, dtype=F64), np.asarray(ref, dtype=F64)
    return float(np.max(np.abs(z - ref) / (1.0 + np.abs(ref)))) if ref.size else 0.0


CL_NOISE_SHAPES = [(2, 20, 1, 3, 5), (1, 64, 2, 4, 4)]


def cl_noise_ref(shape, seed, offset):
    """The channels-last noise kernel's draw in logical (N, C, D, H, W) order: work item i = (n PIX + pix) G + g owns channels 8 g .. 8 g + 7 of pixel pix of sample n
    (csrc/cl_elementwise.hip cl_decode: group fastest, then pixel, then sample); its element e uses counter 2 i + e // 4, word e % 4"""
    N, C, D, H, W = X.five(shape)
    G, PIX = (C + 7) // 8, D * H * W
    z = normals_of_words(philox_words(2 * N * PIX * G, seed, offset)).reshape(N, PIX, G * 8)      # counters 2 i, 2 i + 1 -> the 8 elements of item i, g fastest
    return np.ascontiguousarray(z[:, :, :C].transpose(0, 2, 1)).reshape(N, C, D, H, W)


def half_ulp(ref, dtype):
    """Half a unit in the last place of `dtype` (bf16: 8 significand bits, fp16: 11) at |ref|, fp64"""
    bits = {torch.bfloat16: 8, torch.float16: 11}[dtype]
    emin = {torch.bfloat16: -126, torch.float16: -14}[dtype]
    e = np.floor(np.log2(np.maximum(np.abs(ref), 2.0 ** emin)))
    return 0.5 * 2.0 ** (e - (bits - 1))


# ------------------------------------------------------------------------------------------------------------------------------------------------------
# 3. GAN losses
# ------------------------------------------------------------------------------------------------------------------------------------------------------
LOSS_N = (1, 255, 256, 257, 1000, 4097)
HINGE_KINDS, SOFTPLUS_KINDS = (2, 3), (0, 1, 4)


def loss_logits(n, kind):
    """fp64 logits that are fp32 values.  Hinge kinds: k / 2, k integer in [-8, 8], +-1 planted; softplus kinds: N(0, 3) with +-20, +-88, +-100 planted"""
    g = torch.Generator().manual_seed(X.seed_of(f"loss:{n}:{kind}"))
    if kind in HINGE_KINDS:
        y = torch.randint(-8, 9, (n,), generator=g).double() / 2.0
        plant = [1.0, -1.0]
    else:
        y = (torch.randn(n, generator=g) * 3.0).float().double()
        plant = [20.0, -20.0, 88.0, -88.0, 100.0, -100.0]
    pos = torch.randperm(n, generator=g)[:len(plant)]
    for i, p in zip(pos.tolist(), plant):       # n = 1: the first planted value only
        y[i] = p
    return y.numpy()


def gan_loss_ref(y, kind):
    """-> (per-element loss f, per-element derivative g) in fp64; the value is sum f / n and dy = g / n"""
    v = np.asarray(y, dtype=F64)
    with np.errstate(over="ignore"):
        if kind in (0, 4):
            return np.logaddexp(0.0, -v), -1.0 / (1.0 + np.exp(v))
        if kind == 1:
            return np.logaddexp(0.0, v), 1.0 / (1.0 + np.exp(-v))
    if kind == 2:
        return np.maximum(1.0 - v, 0.0), np.where(1.0 - v > 0, -1.0, 0.0)
    return np.maximum(1.0 + v, 0.0), np.where(1.0 + v > 0, 1.0, 0.0)


def inv32(n):
    return F32(1) / F32(n)


def hinge_expected(y, kind):
    """Bit-exact expectations: loss = float32(sum_f64 / n) (f is a multiple of 1/2 below 8: the fp64 sum is exact in any order), dy = g * (float32(1) / float32(n))"""
    f, g = gan_loss_ref(y, kind)
    assert bool(np.all(f * 2 == np.round(f * 2))) and f.sum() < 2 ** 40
    return F32(F64(f.sum()) / F64(len(f))), (g.astype(F32) * inv32(len(f))).astype(F32)


def softplus_bounds(y, kind):
    """-> (loss_ref, bound on |loss - loss_ref|, dy_ref (fp64, g times the fp32 1/n), bound on |dy - dy_ref|), by counting.
    f = fl(max(-+v, 0) + log1pf(expf(-|v|))): with t = exp(-|v|) <= 1, expf is off by EXP_ULPS ulp = 2 EXP_ULPS U t (plus TINY where it leaves the normal range),
    log1p has slope <= 1, log1pf adds 2 LOG1P_ULPS U log1p(t), the sum one rounding U f.  The fp64 accumulation and division carry 2^-53; the value is rounded to
    fp32 once (U |loss|).
    g = -+1 / fl(1 + expf(+-v)): the sum s = 1 + e has relative error 2 EXP_ULPS U e / s + U, the quotient 2 DIV_ULPS U, the product with 1/n one rounding; where
    expf overflows g is 0 and the true value below TINY."""
    f, g = gan_loss_ref(y, kind)
    n = len(f)
    v = np.asarray(y, dtype=F64)
    t = np.exp(-np.abs(v))
    bf = U * (2 * EXP_ULPS * t + 2 * LOG1P_ULPS * np.log1p(t) + f) + TINY
    loss = f.sum() / n
    with np.errstate(over="ignore"):
        e = np.exp(v if kind in (0, 4) else -v)
        frac = np.where(np.isinf(e), 1.0, e / (1.0 + e))
    rel = (2 * EXP_ULPS * frac + 1 + 2 * DIV_ULPS + 1) * U
    dy = g * F64(inv32(n))
    return loss, bf.sum() / n * (1 + 2.0 ** -20) + U * abs(loss), dy, np.abs(dy) * rel * (1 + 2.0 ** -10) + TINY


# ------------------------------------------------------------------------------------------------------------------------------------------------------
# 4. GRU
# ------------------------------------------------------------------------------------------------------------------------------------------------------
GRU_SHAPES = [(1, 1, 1), (5, 3, 7), (16, 5, 10), (3, 2, 32), (4, 70, 31)]      # (T, B, dm)


def gru_layout_operands(T, B, dm):
    """h0[b, u]: distinct small integers; e: random (its weights are zero).  With every weight and bias zero r = z = 1/2 and n = 0, so
    out[b, t, u] = h0[b, u] 2^-(t + 1) exactly."""
    g = torch.Generator().manual_seed(X.seed_of(f"gru-layout:{T}:{B}:{dm}"))
    h0 = (torch.arange(B * dm, dtype=torch.float64) + 1.0).view(B, dm)
    e = torch.randn(T, B, dm, generator=g, dtype=torch.float64).float().double()
    out = h0.view(B, 1, dm) * (2.0 ** -(torch.arange(T, dtype=torch.float64) + 1.0)).view(1, T, 1)
    gates = torch.zeros(T, B, 4, dm, dtype=torch.float64)
    gates[:, :, 0:2] = 0.5
    assert bool(X.is_f32(out).all())
    return h0, e, out, gates


def gru_operands(T, B, dm):
    """Random parameters (GRUCell's initialisation: uniform in +-1 / sqrt(dm)), inputs, initial state and output cotangent, fp64 holding fp32 values.  Drawn from a
    generator of its own: the process-wide one is left alone."""
    g = torch.Generator().manual_seed(X.seed_of(f"gru:{T}:{B}:{dm}"))
    r = lambda *s: torch.randn(*s, generator=g).double()
    w = lambda *s: ((torch.rand(*s, generator=g) * 2 - 1) * dm ** -0.5).double()
    return dict(e=r(T, B, dm), h0=r(B, dm), dout=r(B, T, dm), w_ih=w(3 * dm, dm), w_hh=w(3 * dm, dm), b_ih=w(3 * dm), b_hh=w(3 * dm))


def gru_unrolled(o, dtype):
    """torch.nn.GRUCell unrolled over T with autograd, in `dtype` on the CPU -> dict(out (B, T, dm) and the four parameter gradients for the cotangent o["dout"])"""
    T, B, dm = o["e"].shape
    with torch.random.fork_rng(devices=[]):      # the constructor draws an initialisation from the process-wide generator
        cell = torch.nn.GRUCell(dm, dm).to(dtype)
    with torch.no_grad():
        cell.weight_ih.copy_(o["w_ih"]); cell.weight_hh.copy_(o["w_hh"]); cell.bias_ih.copy_(o["b_ih"]); cell.bias_hh.copy_(o["b_hh"])
    e, h = o["e"].to(dtype), o["h0"].to(dtype)
    outs = []
    for t in range(T):
        h = cell(e[t], h)
        outs.append(h)
    out = torch.stack(outs, 1)
    (out * o["dout"].to(dtype)).sum().backward()
    return dict(out=out.detach(), dw_ih=cell.weight_ih.grad, dw_hh=cell.weight_hh.grad, db_ih=cell.bias_ih.grad, db_hh=cell.bias_hh.grad)


def gru_plain(o):
    """The recurrence written out in fp64 (the kernel's formulas) -> (out (B, T, dm), gates (T, B, 4, dm))"""
    T, B, dm = o["e"].shape
    h = o["h0"].clone()
    outs, gates = [], []
    for t in range(T):
        gi = o["e"][t] @ o["w_ih"].t() + o["b_ih"]
        gh = h @ o["w_hh"].t() + o["b_hh"]
        r = torch.sigmoid(gi[:, :dm] + gh[:, :dm])
        z = torch.sigmoid(gi[:, dm:2 * dm] + gh[:, dm:2 * dm])
        hn = gh[:, 2 * dm:]
        n = torch.tanh(gi[:, 2 * dm:] + r * hn)
        h = n + z * (h - n)
        outs.append(h)
        gates.append(torch.stack([r, z, n, hn], 1))
    return torch.stack(outs, 1), torch.stack(gates, 0)


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def gru_passes(e_hip, e_cpu):
    """tests/test_ops_gpu.py::test_wgrad_long_reduction_accuracy's convention"""
    return e_hip < 5 * max(e_cpu, 2e-7)


# ------------------------------------------------------------------------------------------------------------------------------------------------------
# 5. channel softmax / argmax
# ------------------------------------------------------------------------------------------------------------------------------------------------------
SM_SHAPES = [(3, 25, 5, 7, 9), (2, 1, 1, 4, 4), (2, 2, 3, 8, 8)]
SM_GRID = 2.0 ** -10


def sm_layouts(C):
    s = ("slice", C + 3, 2)
    return [("plain", "plain"), ("permuted", "permuted"), (s, s), ("permuted", s), (s, "plain")]      # (inputs, output)


def softmax_operands(shape):
    """Logits N(0, 3) on a 2^-10 grid — so x - max is exact in fp32 also at the position shifted by +1e4, and the roundings the bound counts are all there are —
    with one position of logits +-80 and one shifted by +1e4; dy N(0, 1).  fp64 holding fp32 values."""
    g = torch.Generator().manual_seed(X.seed_of(f"softmax:{shape}"))
    N, C, D, H, W = shape
    x = ((torch.randn(shape, generator=g) * 3.0) / SM_GRID).round().double() * SM_GRID
    x[0, :, 0, 0, 1] = torch.where(torch.arange(C) % 2 == 0, 80.0, -80.0).double()
    x[N - 1, :, D - 1, H - 1, W - 2] += 1e4
    assert bool(X.is_f32(x).all()) and bool(X.is_f32(x - x.max(1, keepdim=True).values).all())
    dy = torch.randn(shape, generator=g).double()
    return x, dy


def softmax_forward_bound(ref):
    """(2 * 3 + C + 2) U relative: expf on numerator and sum, C additions, one divide; TINY where the quotient leaves the normal range"""
    C = ref.shape[1]
    return (2 * 3 + C + 2) * U * ref.abs() + TINY


def softmax_backward_ref(dy, y):
    return y * (dy - (dy * y).sum(1, keepdim=True))


def softmax_backward_bound(dy, y):
    """dx = fl(y fl(dy - dot)), dot a C-term fp32 dot product: |dot - dot_ref| <= (C + 1) U sum |dy y| (C products and C additions, gamma_C+1 of recursive
    summation), the subtraction U |dy - dot|, the product U |dx|; second-order terms in the factor 1 + 2^-10"""
    C = y.shape[1]
    dot = (dy * y).sum(1, keepdim=True)
    b = y.abs() * ((C + 1) * U * (dy * y).abs().sum(1, keepdim=True) + U * (dy - dot).abs()) + U * softmax_backward_ref(dy, y).abs()
    return b * (1 + 2.0 ** -10) + TINY


def argmax_operands(shape):
    """Integer logits in [-3, 3] (ties are the rule) with planted positions: all channels equal, the maximum twice with the first at channel 0, and twice at the
    last two channels"""
    g = torch.Generator().manual_seed(X.seed_of(f"argmax:{shape}"))
    N, C, D, H, W = shape
    x = torch.randint(-3, 4, shape, generator=g).double()
    x[0, :, 0, 0, 0] = 2.0
    x[0, :, 0, 0, 1] = -1.0
    x[0, 0, 0, 0, 1] = 3.0
    x[0, C - 1, 0, 0, 1] = 3.0
    x[0, :, 0, 0, 2] = 0.0
    x[0, C - 1, 0, 0, 2] = 1.0
    x[0, max(C - 2, 0), 0, 0, 2] = 1.0
    return x


def argmax_first(x):
    return torch.from_numpy(np.argmax(x.numpy(), axis=1))      # numpy: the first maximum


def onehot_ref(x):
    idx = argmax_first(x).unsqueeze(1)
    return torch.full_like(x, -1.0).scatter_(1, idx, 1.0)


def palette_of(C):
    return ((np.arange(C * 3, dtype=np.int64) * 37 + 11) % 256).astype(np.uint8).reshape(C, 3)


def segm_rgb_ref(x, palette):
    idx = argmax_first(x).numpy()                               # (N, D, H, W)
    return np.ascontiguousarray(np.moveaxis(palette[idx], -1, 1))      # (N, 3, D, H, W)


# ------------------------------------------------------------------------------------------------------------------------------------------------------
# 6. flow visualisation
# ------------------------------------------------------------------------------------------------------------------------------------------------------
FLOW_SHAPE = (2, 2, 3, 5, 13)      # (B, 2, T, H, W): six frames of 5 x 13
FLOW_SCALE = 5.0
FLOW_MAGS = (0.031, 0.074, 0.118, 0.163, 0.209, 0.256, 0.304, 0.353, 0.403, 0.454, 0.506, 0.559, 0.613, 0.668, 0.724, 0.781, 0.839, 0.898, 0.958)
FLOW_ZERO_FRAME, FLOW_CONST_FRAME, FLOW_CLIP_FRAME = 1, 4, 2
FLOW_SAFE = 1e-3


def flow_operands():
    """Directions (2 k + 1) degrees (the hue bucket's middle), magnitudes from FLOW_MAGS; frame FLOW_ZERO_FRAME all zero, frame FLOW_CONST_FRAME the axis vectors
    (+-1/2, 0), (0, +-1/2) — one magnitude in fp32 as in fp64 — and frame FLOW_CLIP_FRAME with four vectors beyond the clip, (+-2, +-2).  fp32 values in fp64."""
    B, _, T, H, W = FLOW_SHAPE
    f = torch.zeros(FLOW_SHAPE, dtype=torch.float64)
    i = 0
    for bt in range(B * T):
        b, t = divmod(bt, T)
        for p in range(H * W):
            h, w = divmod(p, W)
            if bt == FLOW_ZERO_FRAME:
                v = (0.0, 0.0)
            elif bt == FLOW_CONST_FRAME:
                v = [(0.5, 0.0), (0.0, 0.5), (-0.5, 0.0), (0.0, -0.5)][p % 4]
            elif bt == FLOW_CLIP_FRAME and p < 4:
                v = [(2.0, 2.0), (-2.0, 2.0), (-2.0, -2.0), (2.0, -2.0)][p]
            else:
                k, m = (i * 53 + 7) % 180, FLOW_MAGS[(i * 7 + bt) % len(FLOW_MAGS)]
                a = math.radians(2 * k + 1)
                v = (m * math.cos(a), m * math.sin(a))
                i += 1
            f[b, 0, t, h, w], f[b, 1, t, h, w] = v
    return f.float().double()


def flow_rgb_ref(f, scale=FLOW_SCALE):
    """dcv_flow_to_rgb's contract in fp64: clip to [-1, 1], times scale, magnitude, per-frame min-max, H = floor(deg / 2), V = floor((m - lo) 255 / (hi - lo)) (0 where
    hi == lo), HSV (S = 255) -> RGB by the sector formula, + 0.5 and truncation.  -> (uint8 (B, 3, T, H, W), safe (same shape, bool): the fp64 V and the channel before
    truncation are each at least FLOW_SAFE from an integer)"""
    f = f.numpy()
    x, y = np.clip(f[:, 0], -1, 1) * scale, np.clip(f[:, 1], -1, 1) * scale          # (B, T, H, W)
    mg = np.sqrt(x * x + y * y)
    ang = np.arctan2(y, x)
    ang = np.where(ang < 0, ang + 2 * np.pi, ang)
    hh = np.floor(np.degrees(ang) / 2.0).astype(np.int64) & 255
    lo, hi = mg.min(axis=(2, 3), keepdims=True), mg.max(axis=(2, 3), keepdims=True)
    span = np.where(hi > lo, hi - lo, 1.0)
    vraw = np.where(hi > lo, (mg - lo) * (255.0 / span), 0.0)
    V = np.floor(vraw)
    h6 = hh / 30.0
    sec = np.floor(h6).astype(np.int64) % 6
    fr = h6 - np.floor(h6)
    p_, q_, t_ = np.zeros_like(V), V * (1 - fr), V * fr
    r = np.choose(sec, [V, q_, p_, p_, t_, V])
    g = np.choose(sec, [t_, V, V, q_, p_, p_])
    b = np.choose(sec, [p_, p_, t_, V, V, q_])
    ch = np.stack([r, g, b], 1) + 0.5                                                  # (B, 3, T, H, W)
    off = lambda a: np.abs(a - np.round(a))
    v_safe = (off(vraw) >= FLOW_SAFE) | ~(hi > lo)
    safe = (off(ch) >= FLOW_SAFE) & v_safe[:, None]
    return np.floor(ch).astype(np.uint8), safe
