"""GPU: the augmentation's interpolated warps and saturation through the C ABI, bit for bit against the numpy restatement tests/augwarp.py — forward,
adjoint, fan-in adjoint and the draw — then the module under autograd and the training iteration.  Outputs sit between NaN (or sentinel) guard bands; every case
prints its figures (pytest -s).  Every fp32 operation is rounded on its own in both, so exact equality is the bar, not a tolerance."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

from tests import augwarp as A
from tests import test_augment_cpu as R
from tests import test_augment_gpu as G      # its helpers: layouts, guard bands, the iteration harness

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F32, U32 = np.float32, np.uint32
SHAPES = [(3, 3, 2, 8, 12), (1, 2, 1, 5, 7), (2, 3, 3, 16, 16), (2, 1, 2, 8, 8), (2, 3, 16, 64, 64)]
LAYOUTS = ["contiguous", "btchw-view", "sliced-view"]
MODES = [(False, 0), (False, 1), (True, 0)]      # (colour, vector_channels): geometry, optical-flow geometry, colour
ALL_OPS = ("flip", "translate", "cutout", "colour", "scale", "rotate", "aniso", "subpixel", "saturation")
ids = lambda s: "x".join(map(str, s))


def _lib():
    from dcvgan_amd import native
    return native.lib()


def _canon(a):
    """Bits, with every NaN as one pattern: where a NaN lands is held exactly; the payload an ARITHMETIC operation hands on is the processor's choice (IEEE 754
    leaves it open), and only the exact path, which moves bits, promises it (checked on the identity row)."""
    b = G._bits(a).copy()
    b[np.isnan(np.ascontiguousarray(a))] = 0x7FC00000
    return b


def _modes(shape):
    return [m for m in MODES if shape[1] >= 2 or not m[1]]      # a vector field has two components: vector_channels = 1 is refused on a one-channel clip


def _drawn(n, H, W, seed=4321):
    """Rows of the draw itself with every op on: what the iteration feeds the kernels."""
    return A.draw_ref(n, H, W, 1.0, max(1, W // 8), max(1, H // 8), min(H, W) // 2, 0.5, 1.0, 511, 1.3, 1.25, A.rot_tan_half(45.0), 0.125, 1.0, seed, 1)[0]


def _rows(H, W, big):
    cs, sn = F32(0.75) / F32(1.25), F32(1.0) / F32(1.25)                        # the draw's rotation at t = 1/2
    rot = lambda **kw: A.make_row(warp=1, inv=(cs, sn, 0.3125, -sn, cs, -0.21875), fwd=(cs, -sn, sn, cs), **kw)
    drawn = [[int(v) for v in r] for r in _drawn(2, H, W)]
    turn = lambda d, k: ((k * math.cos(math.radians(d)), -k * math.sin(math.radians(d))), (k * math.sin(math.radians(d)), k * math.cos(math.radians(d))))
    if big:      # the full plane size: one batch — every op at once, and the rotation under saturation
        return [drawn[0], rot(gain=1.25, bias=-0.125, s=0.3, cy0=20, cx0=-3, cs=17)]
    return [
        A.make_row(),                                                                                                                # 0 identity: bits move
        A.make_row(flip=1, dx=2, dy=-1, gain=0.75, bias=0.5), A.affine_row(((-1, 0), (0, 1)), (2, -1), flip=1, dx=2, dy=-1, gain=0.75, bias=0.5),   # 1, 2: equal by ==
        A.affine_row(((2, 0), (0, 2)), (0.375, -0.25), gain=1.5, bias=0.25), A.affine_row(((0.5, 0), (0, 0.5)), (0, 0.5), gain=0.625),      # 3, 4 scale 2, 1/2
        rot(gain=1.25, bias=-0.125), rot(s=0.3, gain=0.875, bias=0.0625),                                                            # 5, 6 rotation; + saturation
        drawn[0], drawn[1],                                                                                                          # 7, 8 all ops at once
        A.affine_row(((1, 0), (0, 1)), (3 * W, 0.25), gain=2.0, bias=1.0),                                                           # 9 the whole plane goes outside
        A.affine_row(((1, 0), (0, 1)), (0.5, 0.5), cy0=H // 2, cx0=W // 2, cs=2, gain=1.125),                                        # 10 a cutout that covers a tap
        A.make_row(flip=1, dx=-1, dy=1, cy0=1, cx0=2, cs=3, gain=1.375, bias=-0.25, s=1.7),                                          # 11 the exact path + saturation
        A.make_row(warp=1, inv=(float("nan"), 0, 0, 0, 1, 0), fwd=(1, 0, 0, 1)),                                                     # 12 non-finite coordinates give 0
        A.affine_row(((1, 0), (0, 1)), (0, 0.5), gain=1.0),                                                                          # 13 integer in x: two taps of weight 0
        A.affine_row(turn(30.0, 2.0), (0.3, -0.2), gain=1.25, bias=0.5, s=0.7), A.affine_row(turn(20.0, 2.0), (0, 0), gain=0.8),      # 14, 15 scale 2, turned: up to 18 hits
    ]


@functools.lru_cache(maxsize=None)
def _case(shape):
    """Inputs, tables and the restatement's results for one shape, computed once and shared by the layouts and the tests."""
    B, Cc, T, H, W = shape
    rng = np.random.default_rng(sum(shape))
    rows = _rows(H, W, big=H * W * T > 4096)
    rows += [A.make_row()] * (-len(rows) % B)
    n = len(rows)
    table = A.make_table(rows)
    x, g = G._data(rng, (n, Cc, T, H, W)), G._data(rng, (n, Cc, T, H, W))
    if n > 2:
        x[2], g[2] = x[1], g[1]                  # rows 1 and 2: the same map through the exact path and through the taps
        x[0, 0, 0, 0, 0] = -0.0                  # the identity row moves bits: -0.0 and a NaN payload survive on the geometry stream
        x.view(U32)[0, 0, 0, 0, 1] = 0x7FC12345
        x.view(U32)[13, 0, 0, 2, 3] = 0x7FC00001      # a NaN source pixel under row 13 (and under the padding's identity rows nothing else)
    ref = {}
    for colour, vec in _modes(shape):
        ref[("fwd", colour, vec)] = A.forward_ref(x, table, colour, vec)
        ref[("bwd", colour, vec)] = A.backward_ref(g, table, colour, vec)
    return dict(rows=rows, table=table, x=x, g=g, ref=ref, n=n)


def _place(a: np.ndarray, layout: str) -> torch.Tensor:
    if layout != "sliced-view":
        return G._place(a, layout)
    t = torch.from_numpy(np.ascontiguousarray(a))
    B, Cc, T, H, W = t.shape
    buf = torch.full((B, Cc + 1, T, H + 3, W + 5), float("nan"), dtype=torch.float32, device=DEV)
    v = buf[:, 1:, :, 2:2 + H, 3:3 + W]
    v.copy_(t)
    return v


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_warp_apply_and_backward_bit_for_bit(shape, layout):
    from dcvgan_amd import native
    case = _case(shape)
    B = shape[0]
    bad, checked, n0 = [], 0, native.launch_count()
    got_all = {}
    for colour, vec in _modes(shape):
        for direction, src in (("fwd", case["x"]), ("bwd", case["g"])):
            want = case["ref"][(direction, colour, vec)]
            outs = []
            for i in range(0, case["n"], B):
                x = _place(src[i:i + B], layout)
                table = torch.from_numpy(case["table"][i:i + B]).to(DEV)
                out = G._Guarded(x.shape, 1 if layout == "sliced-view" else 0)
                G._call("dcv_aug_warp_apply" if direction == "fwd" else "dcv_aug_warp_apply_backward", x, table, out.view, colour, vec)
                got = out.numpy()
                assert out.intact(), f"{direction} wrote outside its output ({shape}, {layout}, rows {i}..{i + B - 1})"
                same = _canon(got) == _canon(want[i:i + B])
                if not same.all():
                    bad.append((direction, colour, vec, i, int((~same).sum())))
                checked += got.size
                outs.append(got)
            got_all[(direction, colour, vec)] = np.concatenate(outs)
    print(f"\n[augwarp apply {shape} {layout}] {case['n']} rows x {len(_modes(shape))} streams x 2 directions: {checked} values, {native.launch_count() - n0} launches, "
          f"mismatching batches: {len(bad)}")
    assert not bad, bad[:6]
    if case["n"] > 2:
        for key, y in got_all.items():
            assert np.array_equal(y[1], y[2]), ("the exact path and the taps differ on a pure flip + integer shift", key)      # == on finite data
            assert not y[9].any() and not y[12].any(), key                                                                  # everything outside; non-finite coordinates
        y0 = got_all[("fwd", False, 0)][0]
        assert np.array_equal(G._bits(y0), G._bits(case["x"][0])) and G._bits(y0)[0, 0, 0, 1] == 0x7FC12345 and G._bits(y0)[0, 0, 0, 0] == 0x80000000
        # the NaN source pixel (2, 3) of row 13 (shift (0, 0.5): weights 0.5, 0, 0.5, 0) reaches outputs (2, 3) and (3, 3) only — not through a 0 * NaN
        y13 = got_all[("fwd", False, 0)][13, 0, 0]
        assert sorted(map(tuple, np.argwhere(np.isnan(y13)))) == [(2, 3), (3, 3)]
        if shape[1] == 1:      # saturation is ignored unless C == 3 ...
            t1 = case["table"].copy()
            t1[:, 19] = R.ONE_BITS
            assert np.array_equal(_canon(A.forward_ref(case["x"], t1, True)), _canon(got_all[("fwd", True, 0)]))
        if shape[1] == 3:      # ... and acts on RGB; the vector mix acts on C >= 2
            assert not np.array_equal(got_all[("fwd", True, 0)][6], A.forward_ref(case["x"][6:7], A.make_table([case["rows"][6][:19] + [R.ONE_BITS, 0, 0, 0, 0]]), True)[0])
        if shape[1] >= 2:
            assert not np.array_equal(got_all[("fwd", False, 1)][5], got_all[("fwd", False, 0)][5])
            assert not np.array_equal(got_all[("bwd", False, 1)][5], got_all[("bwd", False, 0)][5])


def test_vector_channels_turn_with_the_warp():
    """A quarter turn of a constant flow field (1, 0): the sampled vectors become L (1, 0) = (l00, l10) = (0, 1); the transpose sends a cotangent (0, 1) back to (1, 0)."""
    row = A.affine_row(((0, -1), (1, 0)), (0, 0))
    table = torch.from_numpy(A.make_table([row])).to(DEV)
    x = np.zeros((1, 2, 1, 8, 8), dtype=F32)
    x[0, 0] = 1.0
    out, back = G._Guarded(x.shape), G._Guarded(x.shape)
    G._call("dcv_aug_warp_apply", torch.from_numpy(x).to(DEV), table, out.view, False, 1)
    y = out.numpy()
    assert np.array_equal(G._bits(y), G._bits(A.forward_ref(x, table.cpu().numpy(), False, 1))) and out.intact()
    assert (y[0, 0] == 0).all() and (y[0, 1] == 1).all()
    g = np.zeros_like(x)
    g[0, 1] = 1.0
    G._call("dcv_aug_warp_apply_backward", torch.from_numpy(g).to(DEV), table, back.view, False, 1)
    d = back.numpy()
    assert np.array_equal(G._bits(d), G._bits(A.backward_ref(g, table.cpu().numpy(), False, 1))) and back.intact()
    assert (d[0, 0] == 1).all() and (d[0, 1] == 0).all()


@pytest.mark.parametrize("shape", SHAPES[:4], ids=ids)
def test_warp_fan_in_adjoint_bit_for_bit(shape):
    """dcv_aug_warp_fan_backward: ((base + A^T dy0) + A^T dy1) + A^T embed(dyf) in that order; under identity rows it is ops.fan_out's sum, bit for bit."""
    from dcvgan_amd import native, ops
    B, Cc, T, H, W = shape
    case = _case(shape)
    rng = np.random.default_rng(11)
    frame, bad, launches = T - 1, [], 0
    vecs = (0, 1) if Cc >= 2 else (0,)
    combos = [(True, 2, True), (False, 2, False), (True, 1, False), (False, 1, True)]      # (base, whole cotangents, frame cotangent)
    streams = [(0, v) for v in vecs] + [(1, 0)]      # (colour, vector_channels); the iteration's fan-in is the geometry clip's, the entry takes either stream
    dd = lambda t: (native.ptr(t), C.byref(native.dims5(t))) if t is not None else (None, None)
    for i in range(0, case["n"], B):
        tnp = case["table"][i:i + B]
        table = torch.from_numpy(tnp).to(DEV)
        base, d0, d1 = (G._data(rng, shape) for _ in range(3))
        df = G._data(rng, (B, Cc, H, W))
        for colour, vec in streams:
            for has_base, nfull, has_frame in combos:
                want = A.fan_backward_ref(base if has_base else None, [d0, d1][:nfull], df if has_frame else None, frame, tnp, bool(colour), vec)
                tb = _place(base, "btchw-view") if has_base else None
                t0, t1 = _place(d0, "sliced-view"), (torch.from_numpy(d1).to(DEV) if nfull > 1 else None)
                tf = torch.from_numpy(df).to(DEV).unsqueeze(2) if has_frame else None
                out = torch.full((B, T, Cc, H, W), float("nan"), dtype=torch.float32, device=DEV).permute(0, 2, 1, 3, 4)
                od = native.dims5(out)
                n0 = native.launch_count()
                rc = _lib().dcv_aug_warp_fan_backward(*dd(tb), *dd(t0), *dd(t1), *dd(tf), frame, native.ptr(table), B, native.ptr(out), C.byref(od), colour, vec,
                                                      native.stream_ptr())
                assert rc == 0, _lib().dcv_last_error()
                launches += native.launch_count() - n0
                if not np.array_equal(G._bits(out.cpu().numpy()), G._bits(want)):
                    bad.append((i, colour, vec, has_base, nfull, has_frame))
    # identity rows against the un-augmented fan-in itself
    x = G._place(G._data(rng, shape), "btchw-view").requires_grad_(True)
    gs = [torch.from_numpy(G._data(rng, (B, Cc, H, W))).to(DEV)] + [torch.from_numpy(G._data(rng, shape)).to(DEV) for _ in range(3)]
    (want_t,) = torch.autograd.grad(ops.fan_out(x, frame, 3), [x], gs)
    ident = torch.from_numpy(A.make_table([A.make_row()] * B)).to(DEV)
    got = torch.empty_strided(x.shape, x.stride(), dtype=torch.float32, device=DEV)
    od = native.dims5(got)
    assert _lib().dcv_aug_warp_fan_backward(*dd(gs[1]), *dd(gs[2]), *dd(gs[3]), *dd(gs[0].unsqueeze(2)), frame, native.ptr(ident), B, native.ptr(got), C.byref(od), 0, 0,
                                            native.stream_ptr()) == 0
    print(f"\n[augwarp fan-in {shape}] {case['n']} rows x {len(streams)} streams x {len(combos)} operand sets, {launches} launches (one each), mismatches {len(bad)}")
    assert launches == (case["n"] // B) * len(streams) * len(combos)
    assert not bad, bad[:6]
    assert torch.equal(got.view(torch.int32), want_t.view(torch.int32)), "under the identity the fused fan-in is not ops.fan_out's sum"


@pytest.mark.parametrize("shape", [(2, 2, 2, 7, 9), (2, 3, 2, 64, 64)], ids=ids)
def test_identity_extension_tables_give_the_exact_entries_bits(shape):
    """Every row of the exact path's own test set, widened by the identity extension: the (B, 24) entries return what the (B, 8) entries return."""
    B, Cc, T, H, W = shape
    rng = np.random.default_rng(3)
    rows = R._rows(H, W)
    rows += [dict()] * (-len(rows) % B)
    n = len(rows)
    gains, biases = (rng.standard_normal(n) * 2).astype(F32), rng.standard_normal(n).astype(F32)
    t8 = R.make_table(rows, gains, biases)
    t24 = np.concatenate([t8, np.tile(np.array(A.IDENTITY_EXT, dtype=np.int64).astype(np.int32), (n, 1))], 1)
    x = G._data(rng, (n, Cc, T, H, W))
    x[0, 0, 0, 0, 0] = -0.0
    x.view(U32)[0, 0, 0, 0, 1] = 0x7FC12345
    worst = 0
    from dcvgan_amd import native
    dd = lambda t: (native.ptr(t), C.byref(native.dims5(t)))
    for i in range(0, n, B):
        xt = G._place(x[i:i + B], "btchw-view")
        a, b = torch.from_numpy(t8[i:i + B]).to(DEV), torch.from_numpy(t24[i:i + B]).to(DEV)
        for colour, neg, vec in ((False, -1, 0), (False, 0, 1), (True, -1, 0)):
            for name in ("apply", "apply_backward"):
                o8, o24 = G._Guarded(xt.shape), G._Guarded(xt.shape)
                G._call("dcv_aug_" + name, xt, a, o8.view, colour, neg)
                G._call("dcv_aug_warp_" + name, xt, b, o24.view, colour, vec)
                assert o24.intact()
                worst += int((G._bits(o8.numpy()) != G._bits(o24.numpy())).sum())
            # ... and the fan-in entries: base + two whole cotangents + the frame's, into the generators' layout
            fr = G._place(x[i:i + B, :, :1], "contiguous")
            outs = [torch.full((B, T, Cc, H, W), float("nan"), dtype=torch.float32, device=DEV).permute(0, 2, 1, 3, 4) for _ in range(2)]
            for name, tab, ch, out in (("dcv_aug_fan_backward", a, neg, outs[0]), ("dcv_aug_warp_fan_backward", b, vec, outs[1])):
                od = native.dims5(out)
                rc = getattr(_lib(), name)(*dd(xt), *dd(xt), *dd(xt), *dd(fr), T - 1, native.ptr(tab), B, native.ptr(out), C.byref(od), int(colour), ch, native.stream_ptr())
                assert rc == 0, _lib().dcv_last_error()
            worst += int((G._bits(outs[0].cpu().numpy()) != G._bits(outs[1].cpu().numpy())).sum())
    assert worst == 0


# ---- the table ----------------------------------------------------------------------------------------------------------------------------------------------
LIMITS = dict(G.LIMITS, mask=511, scale_max=1.3, aniso_max=1.25, rot_max_deg=45.0, frac=0.125, sat=1.0)


def _draw(B, H, W, state, seed, offset, lim=LIMITS):
    from dcvgan_amd import native
    n = B * A.ROW_WORDS
    buf = torch.full((n + 2 * G.BAND,), G.SENTINEL, dtype=torch.int32, device=DEV)
    table = buf[G.BAND:G.BAND + n].view(B, A.ROW_WORDS)
    l = native.AugLimits(lim["mx"], lim["my"], lim["size"], lim["mask"] & 15, lim["contrast"], lim["brightness"])
    wl = native.AugWarpLimits(lim["scale_max"], lim["aniso_max"], math.tan(math.radians(lim["rot_max_deg"]) / 2.0), lim["frac"], lim["sat"], lim["mask"] & 496)
    rc = _lib().dcv_aug_warp_draw(native.ptr(table), B, H, W, native.ptr(state), C.byref(l), C.byref(wl), seed, offset, native.stream_ptr())
    assert rc == 0, _lib().dcv_last_error()
    out = table.cpu().numpy()
    assert bool((buf[:G.BAND] == G.SENTINEL).all()) and bool((buf[G.BAND + n:] == G.SENTINEL).all()), "the draw wrote outside its table"
    return out


def _draw_ref(B, H, W, p, seed, offset, lim=LIMITS):
    return A.draw_ref(B, H, W, p, lim["mx"], lim["my"], lim["size"], lim["contrast"], lim["brightness"], lim["mask"], lim["scale_max"], lim["aniso_max"],
                      A.rot_tan_half(lim["rot_max_deg"]), lim["frac"], lim["sat"], seed, offset)


@pytest.mark.parametrize("B", [1, 5, 4096])
def test_warp_draw_bit_for_bit(B):
    H, W = 64, 48
    for seed, offset in [(1234, 1), (0xDEADBEEF12345678, (1 << 32) + 5)]:
        for p in (0.0, 0.5, 1.0):
            got = _draw(B, H, W, G._state(p), seed, offset)
            want, gates = _draw_ref(B, H, W, p, seed, offset)
            assert np.array_equal(got, want), (B, seed, offset, p, int((got != want).any(1).sum()), np.argwhere(got != want)[:4].tolist())
            v1 = G._draw(B, H, W, G._state(p), seed, offset)      # dcv_aug_draw's own output for the same (seed, offset, p)
            assert np.array_equal(got[:, :8], v1)
            if p == 0.0:
                assert all(tuple(int(v) for v in r) == A.IDENTITY_ROW for r in got)
            if p == 1.0:
                assert all(bool(g.all()) for g in gates) and got[:, 8].all()
    lim = dict(LIMITS, mask=R.CUTOUT | A.SATURATION | A.ROTATE)      # disabled ops write their identity
    got = _draw(B, H, W, G._state(1.0), 7, 2, lim)
    assert np.array_equal(got, _draw_ref(B, H, W, 1.0, 7, 2, lim)[0]) and not got[:, 11].any() and not got[:, 14].any() and not got[:, :3].any()
    print(f"\n[augwarp draw B = {B}] 2 (seed, offset) pairs x 3 probabilities equal the restatement bit for bit; words 0-7 equal dcv_aug_draw's")


# ---- the module -----------------------------------------------------------------------------------------------------------------------------------------------
def test_module_under_autograd():
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    from dcvgan_amd import augment, native
    _lib()
    rng = np.random.default_rng(2)
    aug = augment.ClipAugment(G._cfg("isogd-flow"), DEV, p=1.0, adaptive=False, seed=77, ops=ALL_OPS)
    assert aug.vector_channels == 1 and aug.warp
    xg_np, xc_np = G._data(rng, (2, 2, 2, 16, 16)), G._data(rng, (2, 3, 2, 16, 16))
    gg_np, gc_np = G._data(rng, (2, 2, 2, 16, 16)), G._data(rng, (2, 3, 2, 16, 16))
    xg, xc = G._place(xg_np, "btchw-view").requires_grad_(True), G._place(xc_np, "btchw-view").requires_grad_(True)
    gg, gc = torch.from_numpy(gg_np).to(DEV), torch.from_numpy(gc_np).to(DEV)
    gf = torch.from_numpy(np.ascontiguousarray(gg_np[:, :, 0])).to(DEV)
    torch.cuda.synchronize()
    n0, m0 = native.launch_count(), augment.launches()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        torch.cuda.set_sync_debug_mode("error")      # (inside the profiler's own start / stop, which synchronise)
        try:
            yg, yc = aug(xg, xc)
            n1 = native.launch_count()
            dg, dc = torch.autograd.grad([yg, yc], [xg, xc], [gg, gc])
            n2 = native.launch_count()
            table = aug.draw(2, 16, 16)
            f_c, f_i, f_v, f_g = aug.fan_geometry(xg, 1, table)
            yc2 = aug.colour(xc, table)
            (dfan,) = torch.autograd.grad([f_c, f_i, f_v, f_g], [xg], [gg, gf, gg, gg])
            (dc2,) = torch.autograd.grad([yc2], [xc], [gc])
            n3 = native.launch_count()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
    kernels = {e.key: e.count for e in prof.key_averages() if e.device_type == DeviceType.CUDA}
    foreign = {k[:160]: n for k, n in kernels.items() if "at::" in k or "torch" in k.lower()}
    assert not foreign, foreign
    assert any("aug_warp_kernel" in k for k in kernels) and any("aug_warp_draw_kernel" in k for k in kernels), sorted(kernels)
    assert not any("aug_rows_kernel" in k or "aug_draw_kernel" in k for k in kernels), sorted(kernels)
    print(f"\n[augwarp module] launches: forward {n1 - n0} (1 draw + 2 applies), backward {n2 - n1}, fan {n3 - n2} (draw, 2 applies, fan-in, adjoint); "
          f"kernels {sorted(k[:40] for k in kernels)}")
    assert (n1 - n0, n2 - n1, n3 - n2) == (3, 2, 5)
    assert augment.launches() - m0 == native.launch_count() - n0
    lim = aug.limits(16, 16)
    seed = (77 + augment.SEED_SALT) & 0xFFFFFFFFFFFFFFFF
    t1, t2 = (A.draw_ref(2, 16, 16, 1.0, lim.mx, lim.my, lim.size, lim.contrast, lim.brightness, 511, 1.3, 1.25, A.rot_tan_half(45.0), 0.125, 1.0, seed, o)[0] for o in (1, 2))
    assert np.array_equal(table.cpu().numpy(), t2) and tuple(table.shape) == (2, 24)
    for got, want in [(yg, A.forward_ref(xg_np, t1, False, 1)), (yc, A.forward_ref(xc_np, t1, True)), (dg, A.backward_ref(gg_np, t1, False, 1)),
                      (dc, A.backward_ref(gc_np, t1, True)), (yc2, A.forward_ref(xc_np, t2, True)), (dc2, A.backward_ref(gc_np, t2, True)),
                      (f_v, A.forward_ref(xg_np, t2, False, 1)), (dfan, A.fan_backward_ref(gg_np, [gg_np, gg_np], gg_np[:, :, 0], 1, t2, False, 1))]:
        assert np.array_equal(G._bits(got.detach().cpu().numpy()), G._bits(want))
    assert yg.is_contiguous() and dg.stride() == xg.stride() and dc.stride() == xc.stride() and dfan.stride() == xg.stride()
    # refusals before any launch: a table whose width does not fit the entry, either way; colour with vector channels
    narrow = torch.from_numpy(R.make_table([dict(), dict()])).to(DEV)
    v1 = augment.ClipAugment(G._cfg(), DEV, p=1.0, adaptive=False, seed=3)
    n4, c0 = native.launch_count(), aug.rng._counter
    for bad in (lambda: aug(xg.detach(), xc.detach(), table=narrow), lambda: v1(xc.detach()[:, :1], xc.detach(), table=table), lambda: augment.apply(xc.detach(), table, True),
                lambda: augment.warp_apply(xc.detach(), narrow, True), lambda: augment.warp_apply_backward(xc.detach(), narrow, True),
                lambda: augment.warp_apply(xg.detach(), table, True, 1), lambda: augment.warp_apply(xc.detach()[:, :1], table, False, 1), lambda: aug.fan_geometry(xg, 0, narrow), lambda: aug.colour(xc, narrow)):
        with pytest.raises(native.NativeError):
            bad()
    assert native.launch_count() == n4 and aug.rng._counter == c0
    assert np.array_equal(G._bits(augment.warp_apply(xg.detach(), table, False, 1).cpu().numpy()), G._bits(A.forward_ref(xg_np, t2, False, 1)))
    assert np.array_equal(G._bits(augment.warp_apply_backward(gc, table, True).cpu().numpy()), G._bits(A.backward_ref(gc_np, t2, True)))


def test_state_dict_round_trip():
    from dcvgan_amd import augment
    _lib()
    a = augment.ClipAugment(G._cfg(), DEV, p=0.7, adaptive=True, interval=3, seed=5, ops=ALL_OPS, scale_max=1.2, sat=0.5, rot_max_deg=30.0)
    a.draw(4, 64, 64)
    sd = a.state_dict()
    nxt = [a.draw(4, 64, 64).cpu(), a.draw(4, 64, 64).cpu()]
    b = augment.ClipAugment(G._cfg(), DEV, p=0.1, adaptive=False, interval=9, seed=123)
    assert tuple(b.draw(4, 64, 64).shape) == (4, 8)
    b.load_state_dict(sd)
    got = [b.draw(4, 64, 64).cpu(), b.draw(4, 64, 64).cpu()]
    assert tuple(got[0].shape) == (4, 24) and all(torch.equal(x, y) for x, y in zip(nxt, got)) and not torch.equal(nxt[0], nxt[1])
    assert (b.scale_max, b.sat, b.rot_max_deg, b.mask) == (1.2, 0.5, 30.0, 511)


# ---- the iteration --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def runs():
    kw = dict(adaptive=False, seed=31, ops=ALL_OPS)
    return dict(none=G._iterate(2, None), p0=G._iterate(2, dict(kw, p=0.0)), p1a=G._iterate(2, dict(kw, p=1.0)), p1b=G._iterate(2, dict(kw, p=1.0)))


def test_iteration_at_p0_is_the_iteration_without_augmentation(runs):
    none, p0 = runs["none"], runs["p0"]
    print(f"\n[augwarp iteration p = 0] losses {p0['losses'][1]} vs {none['losses'][1]}; launches {p0['launches']} vs {none['launches']}")
    assert p0["aug"].warp and p0["aug"].draws == 6
    assert p0["losses"] == none["losses"]                               # every loss, as Python floats: equal bits
    assert G._same_state(p0["state"], none["state"])                    # every parameter and BatchNorm buffer
    assert p0["model_draws"] == none["model_draws"]


def test_iteration_at_p1(runs):
    none, p0, a, b = runs["none"], runs["p0"], runs["p1a"], runs["p1b"]
    print(f"\n[augwarp iteration p = 1] losses {a['losses'][1]}; launches {a['launches']} vs {none['launches']} without")
    assert a["losses"] == b["losses"] and G._same_state(a["state"], b["state"])      # two runs: the same bits
    assert all(math.isfinite(v) for l in a["losses"] for v in l.values())
    assert a["losses"] != p0["losses"]
    checked = 0
    for n in ("ggen", "cgen"):
        for k, g0 in none["grads"][n].items():
            if g0 is None:
                continue
            g = a["grads"][n][k]
            assert g is not None and bool(torch.isfinite(g).all()) and bool((g != 0).any()), (n, k)
            checked += 1
    assert checked > 20
    aug = a["aug"]
    for it in (1, 2):
        formula = aug.launches_per_iteration(it, taped_phases=2)
        assert formula == 3 + 6 + 2 * 2
        assert a["own"][it - 1] == formula and p0["own"][it - 1] == formula, (a["own"], p0["own"])
        assert p0["launches"][it - 1] == a["launches"][it - 1]      # the table's values change no launch


def test_optical_flow_iteration():
    run = G._iterate(1, dict(adaptive=False, p=1.0, seed=8, ops=ALL_OPS), cfg_name="isogd-flow")
    assert run["aug"].vector_channels == 1 and all(math.isfinite(v) for v in run["losses"][0].values())
