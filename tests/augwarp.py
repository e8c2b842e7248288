"""The NORMATIVE restatement in numpy of the clip augmentation's interpolated warps and saturation: what dcv_aug_warp_draw, dcv_aug_warp_apply,
dcv_aug_warp_apply_backward and dcv_aug_warp_fan_backward compute, bit for bit.  float32 scalars and arrays, ONE rounding per operation (numpy fuses nothing); a unary
minus of the specification is `0 - x`, so an identity row's words are +0.  Words 0-7 of a row and everything about them come from tests/test_augment_cpu.py, the
restatement of the exact path; tests/test_augwarp_cpu.py checks this file, tests/test_augwarp_gpu.py holds the kernels to it with exact equality."""
import math
import struct

import numpy as np

from tests import test_augment_cpu as R

F32, U32 = np.float32, np.uint32
ROW_WORDS = 24
SCALE, ROTATE, ANISO, SUBPIXEL, SATURATION = 16, 32, 64, 128, 256
THIRD = np.array([0x3EAAAAAB], dtype=U32).view(F32)[0]
# The adjoint's candidate box per axis, and the room of its hit list.  The hits of a source pixel are the lattice points of the parallelogram L (-1, 1)^2 about the
# centre; a convex region of area A and perimeter P holds at most A + P / 2 + 1 of them, and the draw's limits (sx, sy <= scale_max * aniso_max <= 2: a rectangle of
# sides 2 sx, 2 sy) give 16 + 8 + 1 = 25: no drawn row loses a hit.  A hand-made row is in contract when 4 |det L| + 2 (|L e1| + |L e2|) + 1 <= 25.
BOX, HITS = 9, 25
ZERO, ONE, HALF = F32(0.0), F32(1.0), F32(0.5)
DEFAULTS = dict(scale_max=1.3, aniso_max=1.25, rot_max_deg=45.0, frac=0.125, sat=1.0)


def f32_bits(v) -> int:
    return struct.unpack("<i", struct.pack("<f", float(v)))[0]


def rot_tan_half(rot_max_deg) -> np.float32:
    """Computed once on the host, in double, then rounded: the device sees only this fp32."""
    return F32(math.tan(math.radians(float(rot_max_deg)) / 2.0))


IDENTITY_EXT = (0, f32_bits(1), 0, 0, 0, f32_bits(1), 0, f32_bits(1), 0, 0, f32_bits(1), f32_bits(1), 0, 0, 0, 0)
IDENTITY_ROW = tuple(R.IDENTITY_ROW) + IDENTITY_EXT


# ---- the draw ------------------------------------------------------------------------------------------------------------------------------------------------
def _vv(w):
    u = R.u01(w)
    return (u + u) - ONE


def _ratio(w, m):
    vv = _vv(w)
    k = (F32(m) - ONE) * np.abs(vv)
    with np.errstate(all="ignore"):
        return np.where(vv >= 0, ONE + k, ONE / (ONE + k)).astype(F32)


def draw_ref(B, H, W, p, mx, my, size, contrast, brightness, mask, scale_max, aniso_max, tan_half, frac, sat, seed, offset):
    """-> ((B, 24) int32, gates): the table dcv_aug_warp_draw writes.  `mask` carries all nine bits; the exact ops' draw sees mask & 15."""
    t8, gates8 = R.draw_ref(B, H, W, p, mx, my, size, contrast, brightness, mask & 15, seed, offset)
    p = F32(p)
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    blocks = []
    for j in range(3):
        idx = np.uint64(4 * B) + np.uint64(4) * np.arange(B, dtype=np.uint64) + np.uint64(j)
        ctr = np.stack([idx & np.uint64(0xFFFFFFFF), idx >> np.uint64(32), np.full(B, offset & 0xFFFFFFFF, np.uint64), np.full(B, offset >> 32, np.uint64)], 1)
        blocks.append(R.philox4x32_10(ctr, key))
    w = lambda j, i: blocks[j][:, i]
    g_scale = bool(mask & SCALE) & (R.u01(w(0, 0)) <= p)
    g_rot = bool(mask & ROTATE) & (R.u01(w(0, 2)) <= p)
    g_aniso = bool(mask & ANISO) & (R.u01(w(1, 0)) <= p)
    g_sub = bool(mask & SUBPIXEL) & (R.u01(w(1, 2)) <= p)
    g_sat = bool(mask & SATURATION) & (R.u01(w(2, 1)) <= p)
    with np.errstate(all="ignore"):
        s_iso = np.where(g_scale, _ratio(w(0, 1), scale_max), ONE).astype(F32)
        t = F32(tan_half) * _vv(w(0, 3))
        tt = t * t
        den = ONE + tt
        cs = np.where(g_rot, (ONE - tt) / den, ONE).astype(F32)
        sn = np.where(g_rot, (t + t) / den, ZERO).astype(F32)
        ra = np.where(g_aniso, _ratio(w(1, 1), aniso_max), ONE).astype(F32)
        sx, sy = s_iso * ra, s_iso / ra
        tx = np.where(g_sub, (F32(frac) * F32(W)) * _vv(w(1, 3)), ZERO).astype(F32)
        ty = np.where(g_sub, (F32(frac) * F32(H)) * _vv(w(2, 0)), ZERO).astype(F32)
        s = np.where(g_sat, ONE + F32(sat) * _vv(w(2, 2)), ONE).astype(F32)
        phi = np.where(t8[:, 0] != 0, F32(-1.0), ONE).astype(F32)
        taux, tauy = t8[:, 1].astype(F32) + tx, t8[:, 2].astype(F32) + ty
        l00, l01, l10, l11 = (cs * sx) * phi, ZERO - sn * sy, (sn * sx) * phi, cs * sy
        a, b, d, e = phi * (cs / sx), phi * (sn / sx), ZERO - sn / sy, cs / sy
        c, f = ZERO - (a * taux + b * tauy), ZERO - (d * taux + e * tauy)
    t = np.zeros((B, ROW_WORDS), dtype=np.int32)
    t[:, :8] = t8
    t[:, 8] = g_scale | g_rot | g_aniso | g_sub
    for i, v in enumerate((a, b, c, d, e, f, l00, l01, l10, l11, s)):
        t[:, 9 + i] = np.ascontiguousarray(v.astype(F32)).view(np.int32)
    return t, gates8 + (g_scale, g_rot, g_aniso, g_sub, g_sat)


def make_row(flip=0, dx=0, dy=0, cy0=0, cx0=0, cs=0, gain=1.0, bias=0.0, warp=0, inv=(1, 0, 0, 0, 1, 0), fwd=(1, 0, 0, 1), s=1.0):
    """One hand-made 24-word row.  inv = (a, b, c, d, e, f); fwd = (l00, l01, l10, l11), the caller's inverse of [[a, b], [d, e]]."""
    return [int(flip), int(dx), int(dy), int(cy0), int(cx0), int(cs), f32_bits(gain), f32_bits(bias), int(warp)] + [f32_bits(v) for v in inv] + \
           [f32_bits(v) for v in fwd] + [f32_bits(s), 0, 0, 0, 0]


def affine_row(L, tau, **kw):
    """A warp row for p_out = L p_src + tau (centred coordinates), the inverse taken in double: exact for the dyadic maps the tests use."""
    (l00, l01), (l10, l11) = L
    det = l00 * l11 - l01 * l10
    a, b, d, e = l11 / det, -l01 / det, -l10 / det, l00 / det
    c, f = -(a * tau[0] + b * tau[1]), -(d * tau[0] + e * tau[1])
    return make_row(warp=1, inv=(a, b, c + 0.0, d, e, f + 0.0), fwd=(l00, l01, l10, l11), **kw)


def make_table(rows):
    return np.array(rows, dtype=np.int64).astype(np.int32).reshape(len(rows), ROW_WORDS)


class _Row:
    def __init__(self, words):
        w = [int(v) for v in words]
        self.flip, self.dx, self.dy, self.cy0, self.cx0, self.cs = w[0] != 0, w[1], w[2], w[3], w[4], w[5]
        self.gain, self.bias = R.bits_f32(w[6]), R.bits_f32(w[7])
        self.warp = w[8] != 0
        self.a, self.b, self.c, self.d, self.e, self.f, self.l00, self.l01, self.l10, self.l11, self.s = (R.bits_f32(v) for v in w[9:20])
        self.v1 = np.array([w[:8]], dtype=np.int64).astype(np.int32)


# ---- the geometry both directions share -----------------------------------------------------------------------------------------------------------------------
def _index(fl, n):
    """floor of a coordinate as an index, clamped to [-2, n] BEFORE the conversion (a NaN takes the lower bound, as fmaxf does)."""
    return np.clip(np.where(np.isnan(fl), F32(-2.0), fl), F32(-2.0), F32(n)).astype(np.int64)


def taps(r, hh, ww, H, W):
    """-> (ok, y0, x0, [w00, w01, w10, w11]) for output pixels (hh, ww): the forward's operations, which the adjoint repeats."""
    cx, cy = F32(W - 1) * HALF, F32(H - 1) * HALF
    with np.errstate(all="ignore"):
        u, v = ww.astype(F32) - cx, hh.astype(F32) - cy
        su = (r.a * u + r.b * v) + r.c
        sv = (r.d * u + r.e * v) + r.f
        sx, sy = su + cx, sv + cy
        ok = np.isfinite(sx) & np.isfinite(sy)
        x0, y0 = np.floor(sx), np.floor(sy)
        fx, fy = sx - x0, sy - y0
        gx, gy = ONE - fx, ONE - fy
        wts = [gy * gx, gy * fx, fy * gx, fy * fx]
    return ok, _index(y0, H), _index(x0, W), wts


def _colour_fwd(v, r, sat):
    """v: (3 or C, ...) source pixels -> the colour step."""
    if sat:
        m = ((v[0] + v[1]) + v[2]) * THIRD
        v = m + r.s * (v - m)
    return (v * r.gain).astype(F32) + r.bias


def _colour_bwd(t, r, sat):
    a = (r.gain * t).astype(F32)
    if sat:
        ma = ((a[0] + a[1]) + a[2]) * THIRD
        a = ma + r.s * (a - ma)
    return a.astype(F32)


def _cut(r, hh, ww):
    return (hh >= r.cy0) & (hh < r.cy0 + r.cs) & (ww >= r.cx0) & (ww < r.cx0 + r.cs)


def _forward_clip(x, r, colour, vec):
    C, T, H, W = x.shape
    sat = bool(colour) and C == 3 and not (r.s == ONE)
    hh, ww = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    with np.errstate(all="ignore"):
        if not r.warp:
            if not sat:
                return R.forward_ref(x[None], r.v1, colour, 0 if vec else -1)[0]
            hs, ws = hh - r.dy, ww - r.dx          # (the restatement of the exact path, with the colour step's saturation in front of gain and bias)
            ok = ~_cut(r, hh, ww) & (hs >= 0) & (hs < H) & (ws >= 0) & (ws < W)
            wsrc = W - 1 - ws if r.flip else ws
            v = x[:, :, np.clip(hs, 0, H - 1), np.clip(wsrc, 0, W - 1)]
            return np.where(ok, _colour_fwd(v, r, True), ZERO).astype(F32)
        ok, y0, x0, wts = taps(r, hh, ww, H, W)
        cut = _cut(r, hh, ww)
        acc = np.zeros(x.shape, dtype=F32)
        for k in range(4):
            ty, tx = y0 + (k >> 1), x0 + (k & 1)
            valid = ok & ~cut & (ty >= 0) & (ty < H) & (tx >= 0) & (tx < W) & (wts[k] != 0)
            v = x[:, :, np.clip(ty, 0, H - 1), np.clip(tx, 0, W - 1)]
            if colour:
                v = _colour_fwd(v, r, sat)
            acc = np.where(valid, acc + (wts[k] * v).astype(F32), acc).astype(F32)
        if vec:
            r0, r1 = acc[0].copy(), acc[1].copy()
            acc[0] = r.l00 * r0 + r.l01 * r1
            acc[1] = r.l10 * r0 + r.l11 * r1
        return np.where(cut, ZERO, acc).astype(F32)


def forward_ref(x, table, colour, vec=0):
    """dcv_aug_warp_apply on a (B, C, T, H, W) float32 array and a (B, 24) table."""
    x = np.asarray(x, dtype=F32)
    assert not (colour and vec) and not (vec and x.shape[1] < 2) and table.shape == (x.shape[0], ROW_WORDS)      # (the entries refuse these)
    return np.stack([_forward_clip(x[b], _Row(table[b]), colour, vec) for b in range(x.shape[0])])


def _backward_clip(g, r, colour, vec, stats=None):
    """stats: a dict that receives `hits`, the (H, W) count of outputs that tap each source pixel, NOT capped at HITS (interpolating rows only)."""
    C, T, H, W = g.shape
    sat = bool(colour) and C == 3 and not (r.s == ONE)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")      # the source pixels
    with np.errstate(all="ignore"):
        if not r.warp:
            if not sat:
                return R.backward_ref(g[None], r.v1, colour, 0 if vec else -1)[0]
            ws = W - 1 - xs if r.flip else xs
            h, w = ys + r.dy, ws + r.dx
            ok = ~_cut(r, h, w) & (h >= 0) & (h < H) & (w >= 0) & (w < W)
            v = g[:, :, np.clip(h, 0, H - 1), np.clip(w, 0, W - 1)]
            return np.where(ok, _colour_bwd(v, r, True), ZERO).astype(F32)
        cx, cy = F32(W - 1) * HALF, F32(H - 1) * HALF
        du, dv = (xs.astype(F32) - cx) - r.c, (ys.astype(F32) - cy) - r.f
        ocx, ocy = (r.l00 * du + r.l01 * dv) + cx, (r.l10 * du + r.l11 * dv) + cy
        ex = np.minimum((np.abs(r.l00) + np.abs(r.l01)) + ONE, F32(4.0)) if not np.isnan(np.abs(r.l00) + np.abs(r.l01)) else F32(4.0)
        ey = np.minimum((np.abs(r.l10) + np.abs(r.l11)) + ONE, F32(4.0)) if not np.isnan(np.abs(r.l10) + np.abs(r.l11)) else F32(4.0)
        fin = np.isfinite(ocx) & np.isfinite(ocy)
        clampi = lambda v, lo, hi: np.clip(np.where(np.isnan(v), F32(lo), v), F32(lo), F32(hi)).astype(np.int64)
        wlo, hlo = clampi(np.ceil(ocx - ex), 0, W), clampi(np.ceil(ocy - ey), 0, H)
        whi = np.minimum(clampi(np.floor(ocx + ex), -1, W - 1), wlo + BOX - 1)
        hhi = np.minimum(clampi(np.floor(ocy + ey), -1, H - 1), hlo + BOX - 1)
        acc = np.zeros(g.shape, dtype=F32)
        nhits, nall = np.zeros((H, W), dtype=np.int64), np.zeros((H, W), dtype=np.int64)
        for i in range(BOX):          # h ascending ...
            for j in range(BOX):      # ... then w ascending
                h, w = hlo + i, wlo + j
                cand = fin & (h <= hhi) & (w <= whi) & ~_cut(r, h, w)
                if not cand.any():
                    continue
                hc, wc = np.clip(h, 0, H - 1), np.clip(w, 0, W - 1)
                ok, y0, x0, wts = taps(r, hc, wc, H, W)
                kx, ky = xs - x0, ys - y0
                sel = (ky * 2 + kx).clip(0, 3)
                wt = np.choose(sel, wts).astype(F32)
                hit = cand & ok & (kx >= 0) & (kx <= 1) & (ky >= 0) & (ky <= 1) & (wt != 0)
                nall += hit
                hit &= nhits < HITS
                t = g[:, :, hc, wc]
                if vec:
                    t = t.copy()
                    d0, d1 = g[0][:, hc, wc], g[1][:, hc, wc]
                    t[0] = r.l00 * d0 + r.l10 * d1
                    t[1] = r.l01 * d0 + r.l11 * d1
                acc = np.where(hit, acc + (wt * t).astype(F32), acc).astype(F32)
                nhits += hit
        if stats is not None:
            stats["hits"] = nall
        return _colour_bwd(acc, r, sat) if colour else acc


def hit_counts(row, H, W):
    """How many outputs tap each source pixel of an H x W plane under one 24-word row (uncapped)."""
    stats = {}
    _backward_clip(np.zeros((1, 1, H, W), dtype=F32), _Row(row), False, 0, stats)
    return stats["hits"]


def backward_ref(g, table, colour, vec=0):
    """dcv_aug_warp_apply_backward: the adjoint, a gather over source pixels."""
    g = np.asarray(g, dtype=F32)
    assert not (colour and vec) and not (vec and g.shape[1] < 2) and table.shape == (g.shape[0], ROW_WORDS)
    return np.stack([_backward_clip(g[b], _Row(table[b]), colour, vec) for b in range(g.shape[0])])


def fan_backward_ref(base, dys, dyf, frame, table, colour, vec=0):
    """dcv_aug_warp_fan_backward: ((base + A^T dys[0]) + A^T dys[1]) + A^T embed(dyf); each A^T term is complete before it is added, absent operands are skipped."""
    r = None if base is None else np.array(base, dtype=F32)
    with np.errstate(all="ignore"):
        for dy in dys:
            term = backward_ref(dy, table, colour, vec)
            r = term if r is None else (r + term).astype(F32)
        if dyf is not None:
            term = backward_ref(np.asarray(dyf, dtype=F32)[:, :, None], table, colour, vec)[:, :, 0]
            if r is None:
                raise ValueError("fan_backward_ref: a frame cotangent alone is not a case of the iteration")
            r[:, :, frame] = (r[:, :, frame] + term).astype(F32)
    return r
