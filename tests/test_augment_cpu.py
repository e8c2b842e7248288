"""CPU: the clip augmentation's binding, and its NORMATIVE restatement in numpy.

The functions below — `philox4x32_10`, `u01`, `draw_ref`, `forward_ref`, `backward_ref`, `observe_ref`, `adjust_ref` — say what dcv_aug_draw, dcv_aug_apply,
dcv_aug_apply_backward, dcv_aug_observe and dcv_aug_adjust compute, bit for bit; tests/test_augment_gpu.py holds the kernels to them with exact equality.  Here the
restatement itself is checked: Philox against the published known-answer vectors, the adjoint identity in exact integers, the gate frequencies of one fixed draw."""
import ctypes
import inspect
import os
import re
import struct

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dcv_aug_apply", "dcv_aug_apply_backward", "dcv_aug_draw", "dcv_aug_observe", "dcv_aug_adjust")
F32, U32 = np.float32, np.uint32
ONE_BITS = struct.unpack("<i", struct.pack("<f", 1.0))[0]
IDENTITY_ROW = (0, 0, 0, 0, 0, 0, ONE_BITS, 0)
FLIP, TRANSLATE, CUTOUT, COLOUR = 1, 2, 4, 8


def f32_bits(v) -> int:
    return struct.unpack("<i", struct.pack("<f", float(v)))[0]


def bits_f32(b) -> np.float32:
    return np.array([int(b) & 0xFFFFFFFF], dtype=U32).view(F32)[0]


# ---- the specification ------------------------------------------------------------------------------------------------------------------------------------
def philox4x32_10(ctr, key):
    """ctr: (N, 4) uint32, key: (2,) -> (N, 4) uint32.  Salmon et al. 2011."""
    c = [np.asarray(ctr, dtype=np.uint64)[:, i].copy() for i in range(4)]
    k0, k1 = int(key[0]), int(key[1])
    m = 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = c[0] * np.uint64(0xD2511F53), c[2] * np.uint64(0xCD9E8D57)
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & np.uint64(m), p1 >> np.uint64(32), p1 & np.uint64(m)
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + 0x9E3779B9) & m, (k1 + 0xBB67AE85) & m
    return np.stack(c, 1).astype(U32)


def u01(r):
    """((float)r + 0.5f) * 2^-32, every operation in fp32: (0, 1]."""
    return (np.asarray(r, dtype=U32).astype(F32) + F32(0.5)) * F32(2.0 ** -32)


def draw_ref(B, H, W, p, mx, my, size, contrast, brightness, mask, seed, offset):
    """-> (B, 8) int32, the table dcv_aug_draw writes.  p: the fp32 in word 0 of the state block."""
    p = F32(p)
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    blocks = []
    for j in range(4):
        idx = 4 * np.arange(B, dtype=np.uint64) + np.uint64(j)
        ctr = np.stack([idx & np.uint64(0xFFFFFFFF), idx >> np.uint64(32), np.full(B, offset & 0xFFFFFFFF, np.uint64), np.full(B, offset >> 32, np.uint64)], 1)
        blocks.append(philox4x32_10(ctr, key))
    w = lambda j, i: blocks[j][:, i]
    g_flip = bool(mask & FLIP) & (u01(w(0, 0)) <= p)
    g_tr = bool(mask & TRANSLATE) & (u01(w(0, 2)) <= p)
    g_cut = bool(mask & CUTOUT) & (u01(w(1, 2)) <= p)
    g_col = bool(mask & COLOUR) & (u01(w(2, 2)) <= p)
    t = np.zeros((B, 8), dtype=np.int64)
    t[:, 0] = g_flip & ((w(0, 1) >> U32(31)) == 1)
    t[:, 1] = np.where(g_tr, (w(1, 0) % U32(2 * mx + 1)).astype(np.int64) - mx, 0)
    t[:, 2] = np.where(g_tr, (w(1, 1) % U32(2 * my + 1)).astype(np.int64) - my, 0)
    t[:, 3] = np.where(g_cut, (w(2, 0) % U32(H)).astype(np.int64) - size // 2, 0)
    t[:, 4] = np.where(g_cut, (w(2, 1) % U32(W)).astype(np.int64) - size // 2, 0)
    t[:, 5] = np.where(g_cut, size, 0)
    gain = F32(1.0) + (F32(2.0) * F32(contrast)) * (u01(w(3, 0)) - F32(0.5))          # two roundings: the product, then the sum
    bias = F32(brightness) * (u01(w(3, 1)) - F32(0.5))
    t[:, 6] = np.where(g_col, gain, F32(1.0)).astype(F32).view(np.int32)
    t[:, 7] = np.where(g_col, bias, F32(0.0)).astype(F32).view(np.int32)
    return t.astype(np.int32), (g_flip, g_tr, g_cut, g_col)


def _row(table, b):
    flip, dx, dy, cy0, cx0, cs, gb, bb = (int(v) for v in table[b])
    return flip != 0, dx, dy, cy0, cx0, cs, bits_f32(gb), bits_f32(bb)


def _negate(v, on):
    bits = np.ascontiguousarray(v).view(U32)
    return (bits ^ U32(0x80000000 if on else 0)).view(F32)


def forward_ref(x, table, colour, neg_ch=-1):
    """dcv_aug_apply on a (B, C, T, H, W) float32 array."""
    x = np.asarray(x, dtype=F32)
    B, C, T, H, W = x.shape
    y = np.zeros(x.shape, dtype=F32)
    hh, ww = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    with np.errstate(all="ignore"):
        for b in range(B):
            flip, dx, dy, cy0, cx0, cs, gain, bias = _row(table, b)
            cut = (hh >= cy0) & (hh < cy0 + cs) & (ww >= cx0) & (ww < cx0 + cs)
            hs, ws = hh - dy, ww - dx
            ok = ~cut & (hs >= 0) & (hs < H) & (ws >= 0) & (ws < W)
            wsrc = W - 1 - ws if flip else ws
            hc, wc = np.clip(hs, 0, H - 1), np.clip(wsrc, 0, W - 1)
            for c in range(C):
                v = _negate(x[b, c][:, hc, wc], flip and c == neg_ch)          # negation is exact
                if colour:
                    v = (v * gain).astype(F32) + bias                          # two separately rounded fp32 operations
                y[b, c] = np.where(ok, v, F32(0.0))                            # (the geometry stream's bits are moved)
    return y


def backward_ref(g, table, colour, neg_ch=-1):
    """dcv_aug_apply_backward: the adjoint, a gather over source pixels."""
    g = np.asarray(g, dtype=F32)
    B, C, T, H, W = g.shape
    out = np.zeros(g.shape, dtype=F32)
    hs, wsrc = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    with np.errstate(all="ignore"):
        for b in range(B):
            flip, dx, dy, cy0, cx0, cs, gain, _ = _row(table, b)
            ws = W - 1 - wsrc if flip else wsrc
            h, w = hs + dy, ws + dx
            cut = (h >= cy0) & (h < cy0 + cs) & (w >= cx0) & (w < cx0 + cs)
            ok = ~cut & (h >= 0) & (h < H) & (w >= 0) & (w < W)
            hc, wc = np.clip(h, 0, H - 1), np.clip(w, 0, W - 1)
            for c in range(C):
                v = _negate(g[b, c][:, hc, wc], flip and c == neg_ch)
                if colour:
                    v = (gain * v).astype(F32)                                 # (sgn * gain) * dy: one rounding
                out[b, c] = np.where(ok, v, F32(0.0))
    return out


def fan_backward_ref(base, dys, dyf, frame, table, colour, neg_ch=-1):
    """dcv_aug_fan_backward: ((base + A^T dys[0]) + A^T dys[1]) + A^T embed(dyf), every addition rounded to fp32, in this order; absent operands are skipped (no
    addition of a zero in their place), and the frame's term only touches frame `frame`."""
    r = None if base is None else np.array(base, dtype=F32)
    with np.errstate(all="ignore"):
        for dy in dys:
            term = backward_ref(dy, table, colour, neg_ch)
            r = term if r is None else (r + term).astype(F32)
        if dyf is not None:
            term = backward_ref(np.asarray(dyf, dtype=F32)[:, :, None], table, colour, neg_ch)[:, :, 0]
            if r is None:
                raise ValueError("fan_backward_ref: a frame cotangent alone is not a case of the iteration")
            r[:, :, frame] = (r[:, :, frame] + term).astype(F32)
    return r


def observe_ref(state, logits):
    """state: list of 8 ints (word 0 = p's bits)."""
    y = np.asarray(logits, dtype=F32).reshape(-1)
    state = list(state)
    state[1] += int((y > 0).sum()) - int((y < 0).sum())       # sign(0) = 0; a NaN counts 0 here ...
    state[2] += int(y.size)                                    # ... and 1 here
    return state


def adjust_ref(state, target, step, p_max):
    state = list(state)
    if state[2] > 0:
        d = state[1] / state[2] - float(target)               # double
        sg = F32(1.0) if d > 0 else (F32(-1.0) if d < 0 else F32(0.0))
        p = bits_f32(state[0]) + sg * F32(step)
        p = min(max(p, F32(0.0)), F32(p_max))
        state[0] = f32_bits(p)
    state[1] = state[2] = 0
    state[3] += 1
    return state


# ---- the binding --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from dcvgan_amd import native
    if not os.path.exists(native.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return native.lib()


def test_new_names_are_bound_declared_and_exported(lib):
    from dcvgan_amd import native
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dcvgan_hip.h")).read(), flags=re.S)
    raw = ctypes.CDLL(native.LIB_PATH)
    for n in NEW:
        assert n in native.EXPORTS, n
        assert re.search(r"\b%s\s*\(" % n, header), f"{n} is not declared in dcvgan_hip.h"
        assert hasattr(raw, n), f"{n} is not exported by the library"
    assert lib.dcv_version() == native.ABI_VERSION == 4
    assert ctypes.sizeof(native.AugLimits) == 24
    assert re.search(r"for f in [^;]*\baugment\b", open(os.path.join(ROOT, "dcvgan_amd", "csrc", "build.sh")).read()), "csrc/augment.hip is not in build.sh's list"


def test_step_runner_argument_defaults_to_none():
    from dcvgan_amd import trainer
    sig = inspect.signature(trainer.StepRunner.__init__)
    assert sig.parameters["augment"].default is None
    assert callable(trainer.build_augment)


def test_refusals_need_no_gpu(lib):
    """Geometry checks run on the host before any launch."""
    from dcvgan_amd import augment, native
    import torch
    from dcvgan_amd.native import Dims5
    fake = ctypes.create_string_buffer(64)      # never dereferenced
    a = ctypes.addressof(fake)
    x = Dims5(2, 3, 2, 8, 8, 384, 128, 64, 8, 1)
    n0 = lib.dcv_launch_count()
    assert lib.dcv_aug_apply(a, ctypes.byref(x), a, 3, a, ctypes.byref(x), 1, -1, None) == native.DCV_EINVAL and b"rows" in lib.dcv_last_error()
    y = Dims5(2, 3, 2, 8, 9, 432, 144, 72, 9, 1)
    assert lib.dcv_aug_apply_backward(a, ctypes.byref(x), a, 2, a, ctypes.byref(y), 1, -1, None) == native.DCV_EINVAL and b"shapes" in lib.dcv_last_error()
    yt = Dims5(2, 3, 2, 8, 8, 384, 64, 192, 8, 1)
    assert lib.dcv_aug_apply(a, ctypes.byref(x), a, 2, a, ctypes.byref(yt), 0, -1, None) == native.DCV_EINVAL and b"contiguous" in lib.dcv_last_error()
    big = Dims5(1, 1, 1, 8, 8192, 65536, 0, 0, 8192, 1)
    assert lib.dcv_aug_apply(a, ctypes.byref(big), a, 1, a, ctypes.byref(big), 0, -1, None) == native.DCV_EUNSUPPORTED
    assert lib.dcv_aug_apply(a, ctypes.byref(x), a, 2, a, ctypes.byref(x), 0, 3, None) == native.DCV_EINVAL
    lim = native.AugLimits(1, 1, 4, 16, 0.5, 1.0)
    assert lib.dcv_aug_draw(a, 2, 8, 8, a, ctypes.byref(lim), 1, 1, None) == native.DCV_EINVAL
    assert lib.dcv_aug_observe(a, 0, a, None) == native.DCV_EINVAL
    assert lib.dcv_aug_adjust(a, 0.6, 0.1, 1.5, None) == native.DCV_EINVAL
    assert lib.dcv_launch_count() == n0
    from dcvgan_amd.configs import CONFIGS
    aug = augment.ClipAugment(CONFIGS["debug-isogd-depth"], "cpu", p=1.0, adaptive=False)
    with pytest.raises(native.NativeError):
        aug(torch.zeros(2, 1, 2, 8, 8), torch.zeros(2, 3, 2, 8, 8))
    assert aug.neg_g == -1 and augment.ClipAugment(CONFIGS["isogd-flow"], "cpu").neg_g == 0
    assert tuple(augment.IDENTITY_ROW) == IDENTITY_ROW
    assert lib.dcv_launch_count() == n0


# ---- the restatement itself -----------------------------------------------------------------------------------------------------------------------------------
def test_philox_known_answers():
    z = philox4x32_10(np.zeros((1, 4), U32), (0, 0))[0]
    assert [f"{int(v):08x}" for v in z] == ["6627e8d5", "e169c58d", "bc57ac4c", "9b00dbd8"]
    o = philox4x32_10(np.full((1, 4), 0xFFFFFFFF, U32), (0xFFFFFFFF, 0xFFFFFFFF))[0]
    assert [f"{int(v):08x}" for v in o] == ["408f276d", "41c83b0e", "a20bc7c6", "6d5451fd"]
    assert u01(np.array([0, 0xFFFFFFFF], U32)).tolist() == [2.0 ** -33, 1.0]


def _rows(H, W):
    """Parameter rows that exercise every branch at a plane of H x W (gain, bias filled in by the caller)."""
    q = max(1, W // 8)
    rows = [
        dict(), dict(flip=1), dict(dx=q), dict(dx=-q), dict(dy=max(1, H // 8)), dict(dy=-max(1, H // 8)), dict(dx=1), dict(dx=-3, flip=1), dict(dx=4 if W > 4 else 2),
        dict(dx=W), dict(dx=-W - 5), dict(dy=H), dict(dx=2 ** 31 - 1, dy=-2 ** 31),
        dict(cy0=-2, cx0=1, cs=4), dict(cy0=H - 2, cx0=W - 3, cs=5), dict(cy0=1, cx0=-3, cs=4), dict(cy0=2, cx0=W - 1, cs=3), dict(cy0=0, cx0=0, cs=H + W),
        dict(cy0=-1, cx0=-1, cs=max(H, W) + 2), dict(cs=-3, cy0=1, cx0=1),
        dict(flip=1, dx=q, dy=-1, cy0=1, cx0=2, cs=max(2, min(H, W) // 2)), dict(flip=1, dx=-2, dy=2, cy0=-1, cx0=W // 2, cs=3), dict(flip=0, dx=-4, dy=1, cy0=H // 2, cx0=-1, cs=4),
    ]
    return rows


def make_table(rows, gains=None, biases=None):
    t = np.zeros((len(rows), 8), dtype=np.int64)
    for i, r in enumerate(rows):
        clamp = lambda v: max(-2 ** 31, min(2 ** 31 - 1, int(v)))
        t[i] = [r.get("flip", 0), clamp(r.get("dx", 0)), clamp(r.get("dy", 0)), r.get("cy0", 0), r.get("cx0", 0), r.get("cs", 0),
                f32_bits(1.0 if gains is None else gains[i]), f32_bits(0.0 if biases is None else biases[i])]
    return t.astype(np.int32)


@pytest.mark.parametrize("shape", [(1, 2, 2, 8, 8), (1, 1, 1, 7, 9), (1, 2, 1, 16, 12)])
def test_adjoint_identity_in_exact_integers(shape):
    """<aug(x), g> == <x, aug^T(g)> with equality in int64: even integers, gain in {0.5, 1, 2}, bias 0."""
    _, C, T, H, W = shape
    rng = np.random.default_rng(7)
    rows = _rows(H, W)
    worst = 0
    for colour in (False, True):
        for neg in (-1, 0):
            for k, gain in enumerate((0.5, 1.0, 2.0)):
                table = make_table(rows, gains=[gain] * len(rows))
                B = len(rows)
                x = (2 * rng.integers(-50, 50, (B, C, T, H, W))).astype(F32)
                g = (2 * rng.integers(-50, 50, (B, C, T, H, W))).astype(F32)
                y, xt = forward_ref(x, table, colour, neg), backward_ref(g, table, colour, neg)
                for b in range(B):
                    lhs, rhs = (y[b].astype(np.float64) * g[b]), (x[b].astype(np.float64) * xt[b])
                    assert np.all(lhs == np.rint(lhs)) and np.all(rhs == np.rint(rhs))
                    l, r = int(lhs.astype(np.int64).sum()), int(rhs.astype(np.int64).sum())
                    assert l == r, (rows[b], colour, neg, gain, l, r)
                    worst = max(worst, abs(l))
    # the identity row moves bits; a whole-plane shift and a whole-plane cutout give zero
    x = rng.standard_normal((3, C, T, H, W)).astype(F32)
    x[0, 0, 0, 0, 0] = -0.0
    x.view(U32)[0, 0, 0, 0, 1] = 0x7FC12345
    t3 = make_table([dict(), dict(dx=W), dict(cs=H + W)])
    y = forward_ref(x, t3, False)
    assert np.array_equal(y[0].view(U32), x[0].view(U32)) and not y[1].any() and not y[2].any()
    print(f"\n[augment adjoint {shape}] {len(rows)} rows x 2 streams x 2 negate x 3 gains, largest |<.,.>| {worst}")


def test_fan_in_restatement_is_the_plain_sum_under_the_identity():
    rng = np.random.default_rng(3)
    shape = (2, 2, 3, 8, 8)
    gc, gv, gg = (rng.standard_normal(shape).astype(F32) for _ in range(3))
    gf = rng.standard_normal((2, 2, 8, 8)).astype(F32)
    want = ((gc + gv) + gg).astype(F32)
    want[:, :, 1] = want[:, :, 1] + gf
    got = fan_backward_ref(gc, [gv, gg], gf, 1, make_table([dict(), dict()]), False)
    assert np.array_equal(got.view(U32), want.view(U32))
    # and it is linear: one adjoint of the sum where sums are exact (small even integers)
    t = make_table([dict(flip=1, dx=2, dy=-1, cy0=1, cx0=2, cs=3), dict(dx=-3, cy0=-1, cx0=5, cs=4)])
    iv, ig = (2.0 * rng.integers(-20, 20, shape)).astype(F32), (2.0 * rng.integers(-20, 20, shape)).astype(F32)
    assert np.array_equal(fan_backward_ref(None, [iv, ig], None, 0, t, False, 0), backward_ref(iv + ig, t, False, 0))


def test_draw_restatement_gate_frequencies_and_ranges():
    """A condition on the layout, not a measurement: B = 4096, p = 0.5, seed 1234, offset 1 — each gate within 5 sqrt(B / 4) = 160 of 2048."""
    B, H, W = 4096, 64, 64
    t, gates = draw_ref(B, H, W, 0.5, 8, 8, 32, 0.5, 1.0, 15, 1234, 1)
    counts = [int(g.sum()) for g in gates]
    flips = int(t[:, 0].sum())
    print(f"\n[augment draw restatement] gates on {counts} of {B} (2048 +- 160), flips {flips} (1024 +- 139)")
    assert all(abs(c - 2048) <= 160 for c in counts), counts
    assert abs(flips - 1024) <= 139
    assert counts == [2104, 2073, 2024, 2024] and flips == 1033
    t0, _ = draw_ref(5, H, W, 0.0, 8, 8, 32, 0.5, 1.0, 15, 1234, 1)
    assert all(tuple(int(v) for v in r) == IDENTITY_ROW for r in t0)
    t1, g1 = draw_ref(B, H, W, 1.0, 8, 8, 32, 0.5, 1.0, 15, 99, 3)
    assert all(bool(g.all()) for g in g1)
    gain, bias = t1[:, 6].copy().view(F32), t1[:, 7].copy().view(F32)
    assert np.abs(t1[:, 1]).max() == 8 and np.abs(t1[:, 2]).max() == 8 and set(t1[:, 5]) == {32}
    assert t1[:, 3].min() >= -16 and t1[:, 3].max() <= 63 - 16 and t1[:, 4].min() >= -16 and t1[:, 4].max() <= 63 - 16
    assert 0.5 < gain.min() and gain.max() <= 1.5 and -0.5 < bias.min() and bias.max() <= 0.5
    # a disabled op writes its identity words even at p = 1
    t2, _ = draw_ref(64, H, W, 1.0, 8, 8, 32, 0.5, 1.0, FLIP | CUTOUT, 99, 3)
    assert not t2[:, 1].any() and not t2[:, 2].any() and set(t2[:, 6]) == {ONE_BITS} and not t2[:, 7].any() and set(t2[:, 5]) == {32}


def test_adjust_restatement():
    s = [f32_bits(0.0), 0, 0, 0, 0, 0, 0, 0]
    s = adjust_ref(observe_ref(s, [1.0, 2.0, -1.0, 0.0, float("nan")]), 0.6, 0.25, 0.5)      # r = 1 / 5 < 0.6: p stays clamped at 0
    assert s[:4] == [f32_bits(0.0), 0, 0, 1]
    s = adjust_ref(observe_ref(s, [1.0] * 4), 0.6, 0.25, 0.4)
    assert bits_f32(s[0]) == F32(0.25)
    s = adjust_ref(observe_ref(s, [1.0] * 4), 0.6, 0.25, 0.4)
    assert bits_f32(s[0]) == F32(0.4)                                                          # clamped at p_max
    s = adjust_ref(s, 0.6, 0.25, 0.4)                                                          # count == 0: p unchanged, adjusts counts
    assert bits_f32(s[0]) == F32(0.4) and s[3] == 4
    s = adjust_ref(observe_ref(s, [1.0, 1.0, 1.0, 1.0, -1.0]), 0.6, 0.25, 0.4)                # r == target exactly (3 / 5 as doubles): unchanged
    assert bits_f32(s[0]) == F32(0.4) and s[1:4] == [0, 0, 5]
