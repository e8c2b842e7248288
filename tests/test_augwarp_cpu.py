"""CPU: the binding of the augmentation's interpolated warps and saturation, and checks of its normative numpy restatement, tests/augwarp.py:
the adjoint identity in exact integers, the saturation's within a derived bound, the draw's composition, frequencies and identities, the constructor's refusals."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from tests import augwarp as A
from tests import test_augment_cpu as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dcv_aug_warp_apply", "dcv_aug_warp_apply_backward", "dcv_aug_warp_fan_backward", "dcv_aug_warp_draw")
F32, U32 = np.float32, np.uint32
LIM = dict(mx=8, my=8, size=32, contrast=0.5, brightness=1.0, mask=511, scale_max=1.3, aniso_max=1.25, tan_half=A.rot_tan_half(45.0), frac=0.125, sat=1.0)


def draw(B, H, W, p, seed, offset, **kw):
    l = dict(LIM, **kw)
    return A.draw_ref(B, H, W, p, l["mx"], l["my"], l["size"], l["contrast"], l["brightness"], l["mask"], l["scale_max"], l["aniso_max"], l["tan_half"], l["frac"],
                      l["sat"], seed, offset)


@pytest.fixture(scope="module")
def lib():
    from dcvgan_amd import native
    if not os.path.exists(native.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return native.lib()


# ---- the binding --------------------------------------------------------------------------------------------------------------------------------------------
def test_new_names_are_bound_declared_and_exported(lib):
    from dcvgan_amd import augment, native
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dcvgan_hip.h")).read(), flags=re.S)
    raw = ctypes.CDLL(native.LIB_PATH)
    for n in NEW:
        assert n in native.EXPORTS, n
        assert re.search(r"\b%s\s*\(" % n, header), f"{n} is not declared in dcvgan_hip.h"
        assert hasattr(raw, n), f"{n} is not exported by the library"
    assert lib.dcv_version() == native.ABI_VERSION == 4                      # added symbols only
    assert ctypes.sizeof(native.AugLimits) == 24 and ctypes.sizeof(native.AugWarpLimits) == 24
    body = re.search(r"typedef struct dcv_aug_warp_limits \{(.*?)\} dcv_aug_warp_limits;", header, flags=re.S).group(1)
    names = [n.strip() for decl in re.findall(r"(?:float|int32_t) ([^;]*);", body) for n in decl.split(",")]
    assert names == [f for f, _ in native.AugWarpLimits._fields_]
    assert tuple(augment.IDENTITY_WARP_ROW) == A.IDENTITY_ROW and augment.WARP_ROW_WORDS == A.ROW_WORDS == 24
    assert {k: augment.OPS[k] for k in ("scale", "rotate", "aniso", "subpixel", "saturation")} == dict(scale=16, rotate=32, aniso=64, subpixel=128, saturation=256)


def test_refusals_need_no_gpu(lib):
    from dcvgan_amd import augment, native
    import torch
    from dcvgan_amd.native import Dims5
    fake = ctypes.create_string_buffer(64)      # never dereferenced
    a = ctypes.addressof(fake)
    x = Dims5(2, 3, 2, 8, 8, 384, 128, 64, 8, 1)
    n0 = lib.dcv_launch_count()
    assert lib.dcv_aug_warp_apply(a, ctypes.byref(x), a, 3, a, ctypes.byref(x), 1, 0, None) == native.DCV_EINVAL and b"rows" in lib.dcv_last_error()
    y = Dims5(2, 3, 2, 8, 9, 432, 144, 72, 9, 1)
    assert lib.dcv_aug_warp_apply_backward(a, ctypes.byref(x), a, 2, a, ctypes.byref(y), 1, 0, None) == native.DCV_EINVAL and b"shapes" in lib.dcv_last_error()
    yt = Dims5(2, 3, 2, 8, 8, 384, 64, 192, 8, 1)
    assert lib.dcv_aug_warp_apply(a, ctypes.byref(x), a, 2, a, ctypes.byref(yt), 0, 0, None) == native.DCV_EINVAL and b"contiguous" in lib.dcv_last_error()
    assert lib.dcv_aug_warp_apply(a, ctypes.byref(x), a, 2, a, ctypes.byref(x), 1, 1, None) == native.DCV_EINVAL and b"vector_channels" in lib.dcv_last_error()
    assert lib.dcv_aug_warp_apply(a, ctypes.byref(x), a, 2, a, ctypes.byref(x), 0, 2, None) == native.DCV_EINVAL
    x1 = Dims5(2, 1, 2, 8, 8, 128, 128, 64, 8, 1)
    assert lib.dcv_aug_warp_apply(a, ctypes.byref(x1), a, 2, a, ctypes.byref(x1), 0, 1, None) == native.DCV_EINVAL and b"two components" in lib.dcv_last_error()
    assert lib.dcv_aug_warp_fan_backward(None, None, None, None, None, None, None, None, 0, a, 2, a, ctypes.byref(x), 0, 0, None) == native.DCV_EINVAL
    lim = native.AugLimits(1, 1, 4, 15, 0.5, 1.0)
    good = native.AugWarpLimits(1.3, 1.25, 0.4, 0.125, 1.0, 496)
    assert lib.dcv_aug_warp_draw(a, 0, 8, 8, a, ctypes.byref(lim), ctypes.byref(good), 1, 1, None) == native.DCV_EINVAL
    for bad in (native.AugWarpLimits(1.7, 1.25, 0.4, 0.125, 1.0, 496), native.AugWarpLimits(0.9, 1.0, 0.4, 0.125, 1.0, 496),
                native.AugWarpLimits(1.3, 1.25, float("inf"), 0.125, 1.0, 496), native.AugWarpLimits(1.3, 1.25, 0.4, 0.125, 1.0, 15),
                native.AugWarpLimits(1.3, 1.25, 0.4, -0.5, 1.0, 496), native.AugWarpLimits(1.3, 1.25, 0.4, 0.125, float("nan"), 496)):
        assert lib.dcv_aug_warp_draw(a, 2, 8, 8, a, ctypes.byref(lim), ctypes.byref(bad), 1, 1, None) == native.DCV_EINVAL and b"warp limits" in lib.dcv_last_error()
    lim16 = native.AugLimits(1, 1, 4, 16, 0.5, 1.0)      # the exact ops' struct still takes mask & 15 only
    assert lib.dcv_aug_warp_draw(a, 2, 8, 8, a, ctypes.byref(lim16), ctypes.byref(good), 1, 1, None) == native.DCV_EINVAL
    assert lib.dcv_launch_count() == n0
    from dcvgan_amd.configs import CONFIGS
    aug = augment.ClipAugment(CONFIGS["debug-isogd-depth"], "cpu", p=1.0, adaptive=False, ops=("flip", "rotate"))
    with pytest.raises(native.NativeError):
        aug(torch.zeros(2, 1, 2, 8, 8), torch.zeros(2, 3, 2, 8, 8))
    assert lib.dcv_launch_count() == n0


def test_constructor_refusals_and_what_stays_as_it_is():
    from dcvgan_amd import augment
    from dcvgan_amd.configs import CONFIGS
    cfg = CONFIGS["debug-isogd-depth"]
    mk = lambda **kw: augment.ClipAugment(cfg, "cpu", adaptive=False, **kw)
    for kw in (dict(scale_max=1.7, aniso_max=1.25), dict(scale_max=2.1, aniso_max=1.0), dict(rot_max_deg=180.0), dict(rot_max_deg=270.0), dict(scale_max=0.9),
               dict(aniso_max=0.5), dict(rot_max_deg=-1.0), dict(frac=-0.1), dict(sat=-0.5), dict(ops=("flip", "shear"))):
        with pytest.raises(ValueError):
            mk(**kw)
    a = mk()                                          # today's object: no new op, today's table, today's keys
    assert not a.warp and a.row_words == 8 and a.mask == 15 and a.limits(64, 64).mask == 15
    assert sorted(a.state_dict()) == sorted(["state", "adaptive", "target", "interval", "p_max", "adjust_clips", "batch", "mask", "max_dx", "max_dy", "cut_size",
                                             "contrast", "brightness", "rng"])
    b = mk(ops=("flip", "translate", "cutout", "colour", "scale", "rotate", "aniso", "subpixel", "saturation"))
    assert b.warp and b.row_words == 24 and b.mask == 511 and b.limits(64, 64).mask == 15 and b.warp_limits().mask == 496
    assert (b.scale_max, b.aniso_max, b.rot_max_deg, b.frac, b.sat) == (1.3, 1.25, 45.0, 0.125, 1.0)
    assert F32(b.warp_limits().rot_tan_half) == A.rot_tan_half(45.0)
    sd = b.state_dict()
    assert set(sd) - set(a.state_dict()) == {"scale_max", "aniso_max", "rot_max_deg", "frac", "sat"}
    c = mk(ops=("saturation",), sat=0.5)
    old = {k: v for k, v in sd.items() if k in a.state_dict()}      # a checkpoint without the new constants loads and keeps the constructor's
    c.load_state_dict(old)
    assert c.mask == 511 and c.sat == 0.5 and c.warp
    c.load_state_dict(dict(sd, sat=0.25))
    assert c.sat == 0.25 and c.scale_max == 1.3
    for bad in (dict(sd, scale_max=1.7), dict(sd, rot_max_deg=180.0), dict(sd, sat=-1.0), dict(sd, mask=1024 | 15)):      # a bad checkpoint is refused on load, whole
        with pytest.raises(ValueError):
            c.load_state_dict(bad)
        assert (c.sat, c.scale_max, c.rot_max_deg, c.mask) == (0.25, 1.3, 45.0, 511)
    assert augment.ClipAugment(CONFIGS["isogd-flow"], "cpu", ops=("rotate",)).vector_channels == 1 and b.vector_channels == 0
    assert b.launches_per_iteration(4, 2) == a.launches_per_iteration(4, 2)


# ---- the restatement: the operator ----------------------------------------------------------------------------------------------------------------------------
def _exact_rows(H, W):
    """Maps whose a..f (and L) are multiples of 1/8: every coordinate is a multiple of 1/16 and every weight a multiple of 1/256."""
    return [
        A.make_row(),
        A.make_row(warp=1),
        A.affine_row(((2, 0), (0, 2)), (0, 0)), A.affine_row(((0.5, 0), (0, 0.5)), (0, 0)),                     # scale 2 and 1/2
        A.affine_row(((2, 0), (0, 2)), (1.5, -0.75)), A.affine_row(((0.5, 0), (0, 0.5)), (0.375, 1.125)),
        A.affine_row(((0, -1), (1, 0)), (0, 0)), A.affine_row(((0, -1), (1, 0)), (0.5, -1.5)),                  # a quarter turn
        A.affine_row(((-1, 0), (0, 1)), (2, -1), flip=1, dx=2, dy=-1),                                          # flip + integer shift through the taps
        A.affine_row(((1, 0), (0, 1)), (0.625, -2.375)),                                                        # a sub-pixel shift
        A.affine_row(((1, -0.5), (0, 1)), (0.25, 0)), A.affine_row(((2, 0), (0, 0.5)), (0, 0.5)),               # a shear; anisotropic
        A.affine_row(((0, -2), (0.5, 0)), (1.25, -0.5), cy0=1, cx0=2, cs=3),                                    # turn + aniso + shift + cutout
        A.affine_row(((1, 0), (0, 1)), (3 * W, 0)), A.affine_row(((1, 0), (0, 1)), (0, -2.5 * H)),              # the whole plane goes outside
        A.affine_row(((1, 0), (0, 1)), (0.5, 0.5), cy0=-1, cx0=-1, cs=max(H, W) + 2),                           # a cutout over everything
        A.make_row(flip=1, dx=1, dy=-2, cy0=2, cx0=1, cs=2),                                                    # the exact path
    ]


@pytest.mark.parametrize("shape", [(3, 1, 6, 7), (2, 2, 8, 8)], ids=lambda s: "x".join(map(str, s)))
def test_adjoint_identity_in_exact_integers(shape):
    """<A x, g> == <x, A^T g> with equality in int64: data in multiples of 1024, weights in multiples of 1/256, gain in {0.5, 1, 2}, s = 1."""
    C, T, H, W = shape
    rng = np.random.default_rng(17)
    rows = _exact_rows(H, W)
    worst = checked = 0
    for colour, vec in ((False, 0), (False, 1), (True, 0)):
        for gain in (0.5, 1.0, 2.0) if colour else (1.0,):
            table = A.make_table(rows)
            table[:, 6] = R.f32_bits(gain)
            B = len(rows)
            x = (1024 * rng.integers(-8, 9, (B, C, T, H, W))).astype(F32)
            g = (1024 * rng.integers(-8, 9, (B, C, T, H, W))).astype(F32)
            y, xt = A.forward_ref(x, table, colour, vec), A.backward_ref(g, table, colour, vec)
            for b in range(B):
                lhs, rhs = y[b].astype(np.float64) * g[b], x[b].astype(np.float64) * xt[b]
                assert np.all(lhs == np.rint(lhs)) and np.all(rhs == np.rint(rhs)), (b, colour, vec)
                l, r = int(lhs.astype(np.int64).sum()), int(rhs.astype(np.int64).sum())
                assert l == r, (b, colour, vec, gain, l, r)
                worst, checked = max(worst, abs(l)), checked + 1
            assert not y[13].any() and not y[14].any() and not y[15].any() and not xt[13].any() and not xt[15].any()
    print(f"\n[augwarp adjoint {shape}] {checked} (row, stream, gain) cases equal in int64, largest |<.,.>| {worst}")
    assert worst > 0


def test_adjoint_identity_with_saturation_within_a_derived_bound():
    """s != 1 puts (1 - s) / 3 into the operator, which no dyadic data makes exact.  The bound is derived, not measured: both sides are sums of the same products
    w * M[c, c'] * gain * x * g with |M| <= (1 + |s|) / 3 + |s| [c == c'] (m, v - m, s (v - m), m + .. as the forward forms them); the forward rounds each product's
    chain at most 13 times (3 for m, 3 for q, 2 for y, 1 weight, 4 accumulations), the adjoint at most 33 (1 + 25 accumulations, 1 gain, 3 + 3), so
    |lhs - rhs| <= (13 + 33) * 2^-24 * sum |products|, evaluated in fp64 (times 1.01 for the second-order terms and the fp32 evaluation of the weights)."""
    rng = np.random.default_rng(23)
    H, W = 6, 7
    rows = [r for r in _exact_rows(H, W)]
    sats = [0.0, 0.25, 0.7, 1.5, 2.0, -0.5]
    worst = 0.0
    for i, row in enumerate(rows):
        s, gain = sats[i % len(sats)], (0.75, 1.0, 1.31)[i % 3]
        row = list(row)
        row[19], row[6] = R.f32_bits(s), R.f32_bits(gain)
        table = A.make_table([row])
        x, g = rng.standard_normal((1, 3, 2, H, W)).astype(F32), rng.standard_normal((1, 3, 2, H, W)).astype(F32)
        y, xt = A.forward_ref(x, table, True), A.backward_ref(g, table, True)
        lhs, rhs = float((y.astype(np.float64) * g).sum()), float((x.astype(np.float64) * xt).sum())
        xa = np.abs(x.astype(np.float64))
        qa = ((1.0 + abs(s)) / 3.0) * xa.sum(1, keepdims=True) + abs(s) * xa                        # |M| |x|
        geo = A.make_table([row[:6] + [R.f32_bits(1.0), 0] + row[8:19] + [R.f32_bits(1.0), 0, 0, 0, 0]])
        ya = A.forward_ref(qa.astype(F32), geo, False).astype(np.float64) * abs(gain)               # the weights, all non-negative, on |M| |x|
        bound = 1.01 * (13 + 33) * 2.0 ** -24 * float((ya * np.abs(g)).sum())
        assert abs(lhs - rhs) <= bound, (i, s, gain, lhs, rhs, bound)
        if bound > 0:
            worst = max(worst, abs(lhs - rhs) / bound)
    print(f"\n[augwarp saturation adjoint] {len(rows)} rows: largest |lhs - rhs| / bound {worst:.3f}")
    # s is ignored unless C == 3, and exactly 1.0 skips the step
    row = list(A.affine_row(((1, 0), (0, 1)), (0.5, 0.25)))
    x1 = rng.standard_normal((1, 1, 1, H, W)).astype(F32)
    t_s, t_1 = A.make_table([row[:19] + [R.f32_bits(0.3)] + row[20:]]), A.make_table([row])
    assert np.array_equal(A.forward_ref(x1, t_s, True).view(U32), A.forward_ref(x1, t_1, True).view(U32))
    x3 = rng.standard_normal((1, 3, 1, H, W)).astype(F32)
    assert not np.array_equal(A.forward_ref(x3, t_s, True), A.forward_ref(x3, t_1, True))


@pytest.mark.parametrize("limits", [(2.0, 1.0, 45.0), (2.0, 1.0, 179.0), (1.6, 1.25, 179.0), (1.25, 1.6, 90.0)], ids=lambda l: "x".join(map(str, l)))
def test_adjoint_identity_on_rows_drawn_at_the_extreme_limits(limits):
    """No admissible row loses a hit.  Rows are drawn with every op on at the largest scale_max * aniso_max the constructor takes (2) and rotations up to just below
    180 degrees; a source pixel is then tapped by up to 18 outputs (4 det L = 16 on average at scale 2), and the mirror's hit room is the lattice-point bound
    A + P / 2 + 1 = 25 of the rectangle L (-1, 1)^2.  (a) the uncapped hit count of every pixel of every row stays within HITS; (b) <A x, g> == <x, A^T g> within
    the derived bound of the saturation test (forward chain 13 roundings on the colour stream / 5 on the geometry stream, adjoint 33 / 26) — a dropped hit is a whole
    product missing, orders of magnitude above it (with a room of 16 the scale-2 rows miss this bar some forty-fold)."""
    scale_max, aniso_max, deg = limits
    H = W = 20
    B = 48
    table, _ = A.draw_ref(B - 2, H, W, 1.0, 2, 2, 8, 0.5, 1.0, 511, scale_max, aniso_max, A.rot_tan_half(deg), 0.125, 1.0, 2024, 7)
    turn = lambda d, k: ((k * math.cos(math.radians(d)), -k * math.sin(math.radians(d))), (k * math.sin(math.radians(d)), k * math.cos(math.radians(d))))
    table = np.concatenate([table, A.make_table([A.affine_row(turn(30.0, 2.0), (0.3, -0.2), gain=1.25, s=0.7), A.affine_row(turn(20.0, 2.0), (0, 0), gain=0.8)])])
    hits = np.stack([A.hit_counts(r, H, W) for r in table])
    rng = np.random.default_rng(31)
    worst = 0.0
    for colour, Cc, kf, kb in ((False, 2, 5, 26), (True, 3, 13, 33)):
        x, g = rng.standard_normal((B, Cc, 1, H, W)).astype(F32), rng.standard_normal((B, Cc, 1, H, W)).astype(F32)
        t = table.copy()
        t[:, 7] = 0                                                                              # bias has no gradient: the identity is the linear part's
        y, xt = A.forward_ref(x, t, colour), A.backward_ref(g, t, colour)
        geo = t.copy()
        geo[:, 6], geo[:, 19] = R.ONE_BITS, R.ONE_BITS
        gain, s = np.abs(t[:, 6].copy().view(F32).astype(np.float64)), np.abs(t[:, 19].copy().view(F32).astype(np.float64))
        xa = np.abs(x.astype(np.float64))
        if colour:
            xa = ((1.0 + s) / 3.0)[:, None, None, None, None] * xa.sum(1, keepdims=True) + s[:, None, None, None, None] * xa      # |M| |x|
            xa = xa * gain[:, None, None, None, None]
        ya = A.forward_ref(xa.astype(F32), geo, False).astype(np.float64)
        for b in range(B):
            lhs, rhs = float((y[b].astype(np.float64) * g[b]).sum()), float((x[b].astype(np.float64) * xt[b]).sum())
            bound = 1.01 * (kf + kb) * 2.0 ** -24 * float((ya[b] * np.abs(g[b])).sum())
            assert abs(lhs - rhs) <= bound, (limits, colour, b, int(hits[b].max()), lhs, rhs, bound)
            worst = max(worst, abs(lhs - rhs) / bound)
    print(f"\n[augwarp adjoint at the limits {limits}] {B} drawn rows x 2 streams: up to {int(hits.max())} hits per source pixel (room {A.HITS}); "
          f"largest |lhs - rhs| / bound {worst:.3f}")
    assert hits.max() <= A.HITS
    assert hits[-2:].max() > 16                                                                  # scale 2 turned by 30 and 20 degrees: what a room of 16 lost


def test_identity_extension_is_the_exact_path_and_forced_warp_equals_it():
    rng = np.random.default_rng(5)
    shape = (4, 3, 2, 8, 12)
    x, g = rng.standard_normal(shape).astype(F32), rng.standard_normal(shape).astype(F32)
    v1_rows = [dict(), dict(flip=1, dx=2, dy=-1), dict(dx=-3, dy=2, cy0=1, cx0=2, cs=4), dict(flip=1)]
    gains, biases = [1.0, 0.5, 1.25, 2.0], [0.0, 0.25, -0.5, 0.125]
    t8 = R.make_table(v1_rows, gains, biases)
    t24 = np.concatenate([t8, np.tile(np.array(A.IDENTITY_EXT, dtype=np.int64).astype(np.int32), (4, 1))], 1)
    forced = []
    for r, gn, bs in zip(v1_rows, gains, biases):
        phi = -1 if r.get("flip") else 1
        forced.append(A.affine_row(((phi, 0), (0, 1)), (r.get("dx", 0), r.get("dy", 0)), gain=gn, bias=bs, **r))
    tf = A.make_table(forced)
    for colour, vec, neg in ((False, 0, -1), (False, 1, 0), (True, 0, -1)):
        y8, d8 = R.forward_ref(x, t8, colour, neg), R.backward_ref(g, t8, colour, neg)
        y24, d24 = A.forward_ref(x, t24, colour, vec), A.backward_ref(g, t24, colour, vec)
        assert np.array_equal(y8.view(U32), y24.view(U32)) and np.array_equal(d8.view(U32), d24.view(U32))
        yf, df = A.forward_ref(x, tf, colour, vec), A.backward_ref(g, tf, colour, vec)
        assert np.array_equal(yf, y8) and np.array_equal(df, d8), (colour, vec)          # == on finite data: the taps' +0 for the exact path's -0
    gc, gv = rng.standard_normal(shape).astype(F32), rng.standard_normal(shape).astype(F32)
    gf = rng.standard_normal((4, 3, 8, 12)).astype(F32)
    assert np.array_equal(A.fan_backward_ref(gc, [gv, g], gf, 1, t24, False).view(U32), R.fan_backward_ref(gc, [gv, g], gf, 1, t8, False).view(U32))


# ---- the restatement: the draw --------------------------------------------------------------------------------------------------------------------------------
def test_draw_words_0_to_7_and_identities():
    B, H, W = 4096, 64, 64
    for p in (0.0, 0.5, 1.0):
        t, gates = draw(B, H, W, p, 1234, 1)
        t8, _ = R.draw_ref(B, H, W, p, 8, 8, 32, 0.5, 1.0, 15, 1234, 1)
        assert np.array_equal(t[:, :8], t8) and not t[:, 20:].any()      # (the mirror takes words 0-7 from the exact path's mirror, so this only pins that it keeps
                                                                         # doing so; the check with content is the GPU's, against dcv_aug_draw's own output)
        if p == 0.0:
            assert all(tuple(int(v) for v in r) == A.IDENTITY_ROW for r in t)
        if p == 1.0:
            assert all(bool(g.all()) for g in gates) and bool(t[:, 8].all())
    # a disabled op writes its identity even at p = 1; warp follows the four geometric gates only
    t, _ = draw(64, H, W, 1.0, 99, 3, mask=R.CUTOUT | R.COLOUR | A.SATURATION)      # (a flip or an integer shift would be composed into words 9-18)
    assert not t[:, 8].any() and all(tuple(int(v) for v in r[9:19]) == A.IDENTITY_EXT[1:11] for r in t) and (t[:, 19] != R.ONE_BITS).any()
    t, _ = draw(64, H, W, 1.0, 99, 3, mask=A.SUBPIXEL)
    assert t[:, 8].all() and set(t[:, 19].tolist()) == {R.ONE_BITS} and set(t[:, 9].tolist()) == {R.ONE_BITS}
    c, f = t[:, 11].copy().view(F32), t[:, 14].copy().view(F32)
    assert np.abs(c).max() <= 8.0 and np.abs(f).max() <= 8.0 and np.abs(c).max() > 4.0      # frac * W = 8 pixels either way


def test_draw_inverse_pair_box_cap_and_ranges():
    B, H, W = 4096, 64, 64
    t, _ = draw(B, H, W, 1.0, 777, 5)
    a, b, c, d, e, f, l00, l01, l10, l11, s = (t[:, 9 + i].copy().view(F32).astype(np.float64) for i in range(11))
    ulp = 2.0 ** -23
    err = np.stack([a * l00 + b * l10 - 1, a * l01 + b * l11, d * l00 + e * l10, d * l01 + e * l11 - 1])
    scale = np.stack([np.abs(a * l00) + np.abs(b * l10), np.abs(a * l01) + np.abs(b * l11), np.abs(d * l00) + np.abs(e * l10), np.abs(d * l01) + np.abs(e * l11)])
    worst = float((np.abs(err) / np.maximum(scale, 1.0)).max() / ulp)
    ext = np.stack([np.abs(l00) + np.abs(l01), np.abs(l10) + np.abs(l11)])
    det = l00 * l11 - l01 * l10
    print(f"\n[augwarp draw] {B} clips, every op on: |[[a,b],[d,e]] L - I| up to {worst:.2f} ulp of the entries' terms; |l| row sums up to {ext.max():.3f} (cap 3); "
          f"|det L| in [{np.abs(det).min():.3f}, {np.abs(det).max():.3f}]; s in [{s.min():.3f}, {s.max():.3f}]")
    assert worst <= 4.0
    assert ext.max() + 1.0 <= 4.0                                                # every drawn L is inside the adjoint's box
    assert np.abs(det).max() <= 1.3 ** 2 * 1.0001 and np.abs(det).min() >= 1.3 ** -2 * 0.9999
    assert 0.0 < s.min() and s.max() <= 2.0
    theta = np.degrees(np.arctan2(-d, e))                                        # d = -(sin / sy), e = cos / sy
    assert np.abs(theta).max() <= 45.0 + 1e-3 and np.abs(theta).max() > 40.0
    # the constructor's extreme: scale_max * aniso_max = 2 and rot_max_deg just below 180
    t, _ = draw(B, H, W, 1.0, 778, 6, scale_max=1.6, aniso_max=1.25, tan_half=A.rot_tan_half(179.0))
    l = [t[:, 15 + i].copy().view(F32).astype(np.float64) for i in range(4)]
    assert max((np.abs(l[0]) + np.abs(l[1])).max(), (np.abs(l[2]) + np.abs(l[3])).max()) + 1.0 <= 4.0


def test_draw_gate_frequencies():
    """A condition on the layout, not a measurement: B = 4096, p = 0.5, seed 1234, offset 1 — each new gate within 5 sqrt(B / 4) = 160 of 2048."""
    B = 4096
    t, gates = draw(B, 64, 64, 0.5, 1234, 1)
    counts = [int(g.sum()) for g in gates[4:]]
    warp = int(t[:, 8].sum())
    print(f"\n[augwarp draw restatement] scale / rotate / aniso / subpixel / saturation gates on {counts} of {B} (2048 +- 160); warp rows {warp} (3840 +- 78)")
    assert all(abs(c - 2048) <= 160 for c in counts), counts
    assert abs(warp - 3840) <= 78                 # 1 - 2^-4 of the clips; 5 sqrt(B * 15 / 256) = 77.5
    assert [int(g.sum()) for g in gates[:4]] == [2104, 2073, 2024, 2024]      # the first four are the exact path's own
