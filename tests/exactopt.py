"""Host side of the bit-exact optimiser checks (tests/test_opt_exact_cpu.py, tests/test_opt_exact_gpu.py): Adam, the gradient guard, the guarded Adam and the EMA
kernels of csrc/elementwise.hip, and the multi-tensor table they share.  NumPy only; no GPU is touched here.

Everything is a transcription of the device code, one NumPy operation per device operation, in the device's number format: fp32 arrays for what the kernels
compute in fp32 (NumPy rounds every operation once and never contracts), Python floats / float64 for what they compute in double.  The one operation NumPy lacks
is the fused multiply-add: `fmaf32` makes it from an exact double product, an error-free sum and a round-to-odd, so that the final conversion to fp32 is the only
rounding that matters.  The table mirror copies the host loop (mt_for_tables), the device's search (mt_where) and the element-to-thread maps of mt_traverse, and
`describe` names a mismatching word by tensor, element, table, slot, block, thread and trip."""
import math
from collections import namedtuple

import numpy as np

F32, F64, I32, U32, I64 = np.float32, np.float64, np.int32, np.uint32, np.int64
MT, MT_BLOCK, NT = 24, 4096, 256                  # ADAM_MT, MT_BLOCK, threads per block
STRIDED, QUAD = "strided", "quad"                 # MT_STRIDED, MT_QUAD_ORDER (the aligned branch visits a thread's elements in QUAD's order)
GRID_CAP = 8192                                   # grid_for(): adam_kernel strides by at most 8192 blocks of 256
# DCV_GUARD_* (include/dcvgan_hip.h)
LOSS_SCALE, GROWTH_TRACKER, GRAD_NORM, CLIP_COEF, FACTOR, SKIPPED, SKIPPED_TOTAL, NONFINITE = range(8)

RAGGED = [1, 2, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8193, 3 * 4096 + 2]


# ------------------------------------------------------------------------------------------------------------------------------------------------------
# 1. fmaf
# ------------------------------------------------------------------------------------------------------------------------------------------------------
def fmaf32(a, b, c):
    """round_fp32(a * b + c) with ONE rounding, elementwise on fp32 operands.

    a * b has at most 48 significant bits and an exponent far inside double's range: the double product p is exact.  s = fl64(p + c) and TwoSum's e give
    p + c = s + e exactly.  Where e != 0 the true sum lies strictly between s and its neighbour on e's side; round-to-odd takes whichever of the two has an odd
    significand (s itself, or that neighbour: the next double in either direction differs from s in the last bit, across a binade boundary too).  A value rounded to
    odd at 53 bits rounds to any format of at most 51 bits, fp32's 24 and its denormals included, as the exact value would (Boldo & Melquiond, "Emulation of FMA
    and correctly rounded sums: proved algorithms using rounding to odd", 2008)."""
    a, b, c = np.broadcast_arrays(np.asarray(a, F32), np.asarray(b, F32), np.asarray(c, F32))
    with np.errstate(all="ignore"):
        p = a.astype(F64) * b.astype(F64)
        cd = c.astype(F64)
        s = p + cd
        bb = s - p                                  # TwoSum (Knuth): exact for any pair of finite doubles whose sum does not overflow
        e = (p - (s - bb)) + (cd - bb)
        fix = np.isfinite(s) & (e != 0) & ((s.view(I64) & 1) == 0)
        up = (e > 0) == (s > 0)                     # towards larger magnitude: the bit pattern grows
        bits = s.view(I64) + np.where(fix, np.where(up, 1, -1), 0).astype(I64)
        return bits.view(F64).astype(F32)


def fmaf32_naive(a, b, c):
    """What is NOT acceptable: the sum rounded to double, then to fp32 (two roundings)"""
    with np.errstate(all="ignore"):
        return (np.asarray(a, F32).astype(F64) * np.asarray(b, F32).astype(F64) + np.asarray(c, F32).astype(F64)).astype(F32)


# ------------------------------------------------------------------------------------------------------------------------------------------------------
# 2. Adam
# ------------------------------------------------------------------------------------------------------------------------------------------------------
AdamK = namedtuple("AdamK", "w1 b2 w2 eps wd step_size bc2_sqrt gscale")      # AdamScalars, in its field order


def adam_scalars(lr, b1, b2, eps, wd, step, gscale):
    """adam_scalars() of the host and guard_adam_prepare_kernel: Python floats (double), each rounded to fp32 once"""
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    return AdamK(*(F32(x) for x in (1.0 - b1, b2, 1.0 - b2, eps, wd, lr / bc1, math.sqrt(bc2), gscale)))


def adam_update(p, g, m, v, k):
    """adam_update of csrc/elementwise.hip on fp32 arrays -> (p, m, v), one rounding per line's operation as on the device (contraction is off there)"""
    p, g, m, v = (np.asarray(x, F32) for x in (p, g, m, v))
    with np.errstate(all="ignore"):
        g = g * k.gscale
        g = g + k.wd * p
        d = g - m
        m = m + k.w1 * d if k.w1 < F32(0.5) else g - d * (F32(1.0) - k.w1)      # at::lerp's two branches
        v = v * k.b2
        v = v + (k.w2 * g) * g                                                   # addcmul_: value * t1 * t2
        denom = np.sqrt(v) / k.bc2_sqrt + k.eps
        p = p + (-k.step_size) * (m / denom)
    assert p.dtype == m.dtype == v.dtype == F32
    return p, m, v


def adam_update64(p, g, m, v, lr, b1, b2, eps, wd, step, gscale=1.0):
    """the same formula in fp64 throughout, scalars unrounded"""
    g = g * gscale + wd * p
    m = m + (1.0 - b1) * (g - m)
    v = b2 * v + (1.0 - b2) * g * g
    p = p - lr / (1.0 - b1 ** step) * m / (np.sqrt(v) / math.sqrt(1.0 - b2 ** step) + eps)
    return p, m, v


def adam_grid(n):
    """adam_kernel's launch: (blocks, trips of the grid-stride loop)"""
    blocks = min(max((n + NT - 1) // NT, 1), GRID_CAP)
    return blocks, (n + blocks * NT - 1) // (blocks * NT)


# ------------------------------------------------------------------------------------------------------------------------------------------------------
# 3. the multi-tensor table
# ------------------------------------------------------------------------------------------------------------------------------------------------------
def mt_blocks(n):
    return (n + MT_BLOCK - 1) // MT_BLOCK


Table = namedtuple("Table", "t0 nt n first_block blocks block0 launched")


def tables(sizes):
    """mt_for_tables: per table of 24 its first tensor, tensor count, element counts, prefix sums of blocks, block count, the blocks of the tables launched
    before it (the guard's block0) and whether it is launched at all (a table without blocks is skipped)"""
    out, before = [], 0
    for t0 in range(0, len(sizes), MT):
        n = list(sizes[t0:t0 + MT])
        fb = [0]
        for x in n:
            fb.append(fb[-1] + mt_blocks(x))
        out.append(Table(t0, len(n), n, fb, fb[-1], before, fb[-1] > 0))
        before += fb[-1]
    return out


def mt_where(first_block, nt, bid):
    """the device's search, as written -> (slot, block of that tensor)"""
    t = 0
    while t + 1 < nt and bid >= first_block[t + 1]:
        t += 1
    return t, bid - first_block[t]


def total_blocks(sizes):
    return sum(mt_blocks(n) for n in sizes)


def block_owner(sizes):
    """every launched block in launch order: (table, slot, tensor, block of the tensor, global partial index block0 + blockIdx), via mt_where"""
    out = []
    for k, tab in enumerate(tables(sizes)):
        if not tab.launched:
            continue
        for bid in range(tab.blocks):
            slot, blk = mt_where(tab.first_block, tab.nt, bid)
            out.append((k, slot, tab.t0 + slot, blk, tab.block0 + bid))
    return out


def elements_of(n, blk, tid, order):
    """the elements of block `blk` of an n-element tensor that thread `tid` handles, in its order (trip = position in the list); `order` STRIDED is mt_strided, QUAD
    both the aligned quad branch (whole quads as one 16-byte access, the last 1..3 one at a time) and MT_QUAD_ORDER"""
    base = blk * MT_BLOCK
    if order == STRIDED:
        out = []
        for e in range(16):
            i = base + e * NT + tid
            if i >= n:
                break
            out.append(i)
        return out
    out = []
    for q in range(4):
        i = base + (q * NT + tid) * 4
        out += [j for j in range(i, i + 4) if j < n]
    return out


def owner_of(j, order):
    """element j of a tensor -> (block of the tensor, thread, trip); the closed form of elements_of"""
    blk, r = divmod(j, MT_BLOCK)
    if order == STRIDED:
        return blk, r % NT, r // NT
    quad, k = divmod(r, 4)
    return blk, quad % NT, (quad // NT) * 4 + k


def describe(sizes, tensor, elem, order=STRIDED):
    """names an element as the kernels reach it"""
    k, slot = divmod(tensor, MT)
    tab = tables(sizes)[k]
    blk, tid, trip = owner_of(elem, order)
    bid = tab.first_block[slot] + blk
    return (f"tensor {tensor} (n = {sizes[tensor]}) element {elem}: table {k} slot {slot}, block {bid} of the launch (block {blk} of the tensor, "
            f"partial {tab.block0 + bid}), thread {tid}, trip {trip} [{order}]")


def describe_single(n, elem):
    blocks, _ = adam_grid(n)
    return f"element {elem} of {n}: block {(elem // NT) % blocks}, thread {elem % NT}, trip {elem // (blocks * NT)} of adam_kernel's grid-stride loop"


# ------------------------------------------------------------------------------------------------------------------------------------------------------
# 4. the gradient guard
# ------------------------------------------------------------------------------------------------------------------------------------------------------
def _per_thread(x, order):
    """(blocks * 4096,) -> (blocks, 256 threads, 16 trips)"""
    nb = x.size // MT_BLOCK
    if order == STRIDED:
        return x.reshape(nb, 16, NT).transpose(0, 2, 1)
    return x.reshape(nb, 4, NT, 4).transpose(0, 2, 1, 3).reshape(nb, NT, 16)


def block_sum(v):
    """block_sum on (..., 256) doubles: the xor butterfly over each wave's 64 lanes, then waves ((0 + 1) + 2) + 3 -> (...,)"""
    v = np.asarray(v, F64).reshape(v.shape[:-1] + (4, 64))
    lane = np.arange(64)
    with np.errstate(all="ignore"):
        for o in (32, 16, 8, 4, 2, 1):
            v = v + v[..., lane ^ o]
        w = v[..., 0]
        return ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]


def guard_partials(gs, aligned=True, order=QUAD):
    """guard_partial_kernel over the tensors gs (fp32 arrays) -> (partials float64, counts uint32), indexed as the kernel stores them (block0 + blockIdx).  `aligned`
    (one bool, or one per tensor) picks the aligned branch; a tensor off the 16-byte grid is visited in `order` — QUAD is the kernel as it stands, STRIDED what
    it was.  A padded element (0) leaves a thread's chain and count as the kernel's `break` / `j < n` does: fmaf(0, 0, ss) = ss for ss >= +0 and for NaN."""
    sizes = [int(np.asarray(g).size) for g in gs]
    al = [aligned] * len(gs) if isinstance(aligned, bool) else list(aligned)
    part, cnt = np.zeros(total_blocks(sizes), F64), np.zeros(total_blocks(sizes), U32)
    seen = np.zeros(part.size, bool)
    for k, slot, t, blk, idx in block_owner(sizes):
        assert not seen[idx]
        seen[idx] = True
    assert seen.all()      # contiguous, each once
    first = {}
    for k, slot, t, blk, idx in block_owner(sizes):
        if blk == 0:
            first[t] = idx
    for t, g in enumerate(gs):
        nb = mt_blocks(sizes[t])
        if nb == 0:
            continue
        x = np.zeros(nb * MT_BLOCK, F32)
        x[:sizes[t]] = np.asarray(g, F32).reshape(-1)
        th = _per_thread(x, QUAD if al[t] else order)
        ss = np.zeros((nb, NT), F32)
        for e in range(16):
            ss = fmaf32(th[:, :, e], th[:, :, e], ss)
        bad = ((th.view(U32) & U32(0x7f800000)) == U32(0x7f800000)).sum(axis=2)
        part[first[t]:first[t] + nb] = block_sum(ss.astype(F64))
        cnt[first[t]:first[t] + nb] = block_sum(bad.astype(F64)).astype(U32)
    return part, cnt


Rule = namedtuple("Rule", "grad_scale max_norm skip_nonfinite dynamic growth backoff growth_interval", defaults=(1.0, 0.0, 1, 0, 2.0, 0.5, 2000))


def guard_decide(partials, counts, rule, state):
    """guard_decide_kernel in double -> the eight state floats after it (fp32 array); `state` is the eight before it"""
    nb = len(partials)
    rows = -(-max(nb, 1) // NT)
    p, c = np.zeros(rows * NT, F64), np.zeros(rows * NT, F64)
    p[:nb], c[:nb] = partials, np.asarray(counts, F64)
    acc, cc = np.zeros(NT, F64), np.zeros(NT, F64)
    with np.errstate(all="ignore"):
        for r in range(rows if nb else 0):      # thread i: partials i, i + 256, ... (0.0 + x = x for the padding's +0 as well)
            live = np.arange(NT) + r * NT < nb
            acc = np.where(live, acc + p[r * NT:(r + 1) * NT], acc)
            cc = np.where(live, cc + c[r * NT:(r + 1) * NT], cc)
        ss, nbad = float(block_sum(acc)), float(block_sum(cc))
        st = np.array(state, F32).copy()
        scale = st[LOSS_SCALE]
        norm = math.sqrt(ss) * rule.grad_scale / float(scale) if ss >= 0 else float("nan")
        bad = nbad > 0.0 or not math.isfinite(ss) or not np.isfinite(F32(norm))
        coef = 1.0
        if not bad and rule.max_norm > 0.0:
            coef = min(1.0, rule.max_norm / (norm + 1e-6))
        skip = bool(bad and rule.skip_nonfinite)
        st[GRAD_NORM] = F32(norm)
        st[CLIP_COEF] = F32(coef)
        st[FACTOR] = F32(rule.grad_scale * coef / float(scale))
        st[SKIPPED] = F32(1.0 if skip else 0.0)
        st[SKIPPED_TOTAL] = st[SKIPPED_TOTAL] + F32(1.0 if skip else 0.0)
        st[NONFINITE] = F32(nbad)
        if rule.dynamic:
            tracker, s = st[GROWTH_TRACKER], scale
            if bad:
                s, tracker = F32(float(s) * rule.backoff), F32(0.0)
            else:
                tracker = tracker + F32(1.0)
                if tracker >= F32(rule.growth_interval):
                    grown = F32(float(s) * rule.growth)
                    if np.isfinite(grown):
                        s = grown
                    tracker = F32(0.0)
            st[LOSS_SCALE], st[GROWTH_TRACKER] = s, tracker
    return st


# ------------------------------------------------------------------------------------------------------------------------------------------------------
# 5. EMA
# ------------------------------------------------------------------------------------------------------------------------------------------------------
def ema_w(t, decay, warmup):
    """ema_prepare_kernel: the weight of update number t (0-based), formed in double and rounded once"""
    d = min(decay, (1.0 + t) / (10.0 + t)) if warmup else decay
    return F32(1.0 - d)


def ema_update(e, s, w):
    """ema_one: fmaf(w, s - e, e)"""
    e, s = np.asarray(e, F32), np.asarray(s, F32)
    with np.errstate(all="ignore"):
        return fmaf32(F32(w), s - e, e)


# ------------------------------------------------------------------------------------------------------------------------------------------------------
# 6. size lists, arenas, mismatch reports
# ------------------------------------------------------------------------------------------------------------------------------------------------------
def counts_list(k):
    """k tensors of sizes 1..7, except (where the list reaches them) a ragged size in the last slot of the first table and one in the first slot of the next"""
    sizes = [1 + (3 * i) % 7 for i in range(k)]
    if k >= MT:
        sizes[MT - 1] = 4097
    if k > MT:
        sizes[MT] = 8193
    return sizes


COUNTS = {k: counts_list(k) for k in (1, 23, 24, 25, 48, 49)}
_r = lambda k, start=0: [1 + (5 * (i + start)) % 7 for i in range(k)]
ZEROS = {
    "first": [0] + _r(5) + [257],
    "last": _r(5) + [4097, 0],
    "three_mid_table": _r(4) + [0, 0, 0] + _r(4, 2) + [1025],
    "slot23": _r(23) + [0] + _r(3, 1),
    "slot24": _r(23) + [4097] + [0] + _r(3, 1),
    "skipped_table": _r(23) + [4097] + [0] * 24 + [8193, 3, 5],
}
LISTS = dict([("ragged", RAGGED)] + [(f"counts{k}", v) for k, v in COUNTS.items()] + [(f"zeros_{k}", v) for k, v in ZEROS.items()])
BAND = 8                          # NaN words on either side of every tensor; a multiple of 4, so an aligned view stays aligned
NAN_WORD = 0x7f800001             # a SIGNALLING NaN: arithmetic quiets it (0x7fc00001), so a kernel that reads a band word and writes its result back changes the word
                                  # (a quiet NaN would come back from Adam's or the EMA's arithmetic with the bits it went in with, and `i > n` for `i >= n` would pass)


def guard_offs(sizes):
    """the guard tests' 4-byte-off tensors: 6, 16 and 26, or the list's last where it is shorter"""
    return sorted({min(i, len(sizes) - 1) for i in (6, 16, 26)})


class Arena:
    """Where the tensors of one case lie in ONE buffer of 32-bit words: a band of BAND NaN words before, between and after them, tensor i starting on a 16-byte boundary
    plus off[i] words.  fill() and gather() move values between the buffer and the concatenation of all tensors' elements (the order every mirror works in)."""

    def __init__(self, sizes, off=()):
        self.sizes = list(sizes)
        off = set(off)
        self.off = [1 if i in off else 0 for i in range(len(self.sizes))]
        self.start, cur = [], 0
        for n, o in zip(self.sizes, self.off):
            s = (cur + BAND + 3) // 4 * 4 + o
            self.start.append(s)
            cur = s + n
        self.words = (cur + BAND + 3) // 4 * 4
        self.total = sum(self.sizes)
        self.index = np.concatenate([np.arange(s, s + n) for s, n in zip(self.start, self.sizes)] + [np.zeros(0, np.int64)]).astype(np.int64)
        self.tensor_of = np.concatenate([np.full(n, i) for i, n in enumerate(self.sizes)] + [np.zeros(0, np.int64)]).astype(np.int64)
        self.first = np.cumsum([0] + self.sizes)[:-1]

    def fill(self, flat):
        buf = np.full(self.words, NAN_WORD, U32).view(F32)
        buf[self.index] = np.asarray(flat, F32)
        return buf

    def gather(self, buf):
        return np.asarray(buf)[self.index]

    def split(self, flat):
        return [flat[a:a + n] for a, n in zip(self.first, self.sizes)]

    def locate(self, word):
        """buffer word -> (tensor, element) or None for a band word"""
        hit = np.nonzero(self.index == word)[0]
        if hit.size == 0:
            return None
        t = int(self.tensor_of[hit[0]])
        return t, int(hit[0] - self.first[t])


def first_mismatch(arena, got_buf, want_buf, order=STRIDED):
    """None if the two buffers agree word for word (bands included), else a description of the first differing word"""
    a, b = np.asarray(got_buf).view(U32), np.asarray(want_buf).view(U32)
    bad = np.nonzero(a != b)[0]
    if bad.size == 0:
        return None
    w = int(bad[0])
    where = arena.locate(w)
    head = f"{bad.size} of {a.size} words differ; first: word {w} got {int(a[w]):#010x} want {int(b[w]):#010x}: "
    if where is None:
        return head + "a guard-band word was written"
    return head + describe(arena.sizes, where[0], where[1], order)


def unique_normal(rng, n, scale=1.0, unique=True):
    """n fp32 normal values times scale (a scalar or an array), no two equal, so that a mis-addressed element cannot match by chance.  unique=False skips the
    redraws (the 2 M-element case: fp32 has too few values near zero for that many, and there neighbours differ, which is what mis-addressing needs)"""
    x = (rng.standard_normal(n) * scale).astype(F32)
    if not unique:
        return x
    for _ in range(64):
        _, idx, cnt = np.unique(x, return_index=True, return_counts=True)
        if idx.size == n and not np.any(x == 0):
            return x
        dup = np.ones(n, bool)
        dup[idx] = False
        dup |= x == 0
        sc = scale[dup] if isinstance(scale, np.ndarray) else scale
        x[dup] = (rng.standard_normal(int(dup.sum())) * sc).astype(F32)
    raise AssertionError("could not make the values distinct")


def per_tensor(sizes, values):
    """one value per tensor -> one per element of the concatenation"""
    return np.repeat(np.asarray(values, F64), sizes)


def adam_case(sizes, seed, nonzero_state, unique=True):
    """p = 0.05 N(0, 1); g = N(0, 1) times a per-tensor magnitude 10^-6 .. 1; m, v zero or random (v > 0)"""
    rng = np.random.default_rng(seed)
    total = sum(sizes)
    p = unique_normal(rng, total, 0.05, unique)
    mags = 10.0 ** -((np.arange(len(sizes)) * 5) % 7).astype(F64)
    g = unique_normal(rng, total, per_tensor(sizes, mags), unique)
    if nonzero_state:
        m = unique_normal(rng, total, per_tensor(sizes, mags) * 0.5, unique)
        v = np.abs(unique_normal(rng, total, per_tensor(sizes, mags), unique)) ** 2
        v = v.astype(F32)
    else:
        m, v = np.zeros(total, F32), np.zeros(total, F32)
    return p, g, m, v


def guard_int_case(sizes, seed):
    """gradients in +-{1..15} times one power of two 2^0 .. 2^-3 per tensor; the sum of squares stays below 2^22 and every partial sum is exact in fp32 and double"""
    rng = np.random.default_rng(seed)
    total = sum(sizes)
    x = rng.integers(1, 16, total).astype(F64) * rng.choice([-1.0, 1.0], total)
    x = (x * per_tensor(sizes, 2.0 ** -(np.arange(len(sizes)) % 4))).astype(F32)
    assert float((x.astype(F64) ** 2).sum()) < 2.0 ** 22
    return x
