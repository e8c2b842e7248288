"""GPU: the clip augmentation through the C ABI, bit for bit against the numpy restatement of tests/test_augment_cpu.py — forward, adjoint, the
fused fan-in adjoint, the table draw, the adaptive probability — then the module under autograd and the training iteration.  Every output sits between NaN (or
sentinel) guard bands; every case prints its figures (pytest -s).  The separately rounded multiply and add make exact equality the bar, not a tolerance."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

from tests import rig
from tests import test_augment_cpu as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F32, U32 = np.float32, np.uint32
BAND = 64      # guard floats on each side of an output (a multiple of 4: the band keeps the output's alignment)
SHAPES = [(3, 3, 2, 8, 8), (2, 1, 3, 16, 12), (2, 2, 2, 7, 9), (2, 3, 2, 64, 64), (1, 1, 1, 128, 128)]
LAYOUTS = ["contiguous", "btchw-view", "base+4B"]


def _lib():
    from dcvgan_amd import native
    return native.lib()


def _bits(a):
    return np.ascontiguousarray(a).view(U32)


def _data(rng, shape):
    """Gaussian fp32 with magnitudes in [2^-10, 2^10]: no subnormals."""
    x = rng.standard_normal(shape).astype(F32)
    return (np.sign(x) + (x == 0)).astype(F32) * np.clip(np.abs(x), F32(2.0 ** -10), F32(2.0 ** 10))


@functools.lru_cache(maxsize=None)
def _case(shape):
    """Inputs, tables and the restatement's results for one shape, computed once and shared by the layouts."""
    B, Cc, T, H, W = shape
    rng = np.random.default_rng(sum(shape))
    rows = R._rows(H, W)
    rows += [dict()] * (-len(rows) % B)      # whole batches: clips of one batch get different rows
    n = len(rows)
    gains = (rng.standard_normal(n) * np.exp2(rng.integers(-12, 12, n))).astype(F32)
    biases = (rng.standard_normal(n) * np.exp2(rng.integers(-12, 12, n))).astype(F32)
    gains[0], biases[0] = 1.0, 0.0           # row 0: the identity row
    table = R.make_table(rows, gains, biases)
    x = _data(rng, (n, Cc, T, H, W))
    xgeo = x.copy()
    xgeo[0, 0, 0, 0, 0] = -0.0               # ... whose bits move on the geometry stream: -0.0 and a NaN payload survive
    xgeo.view(U32)[0, 0, 0, 0, 1] = 0x7FC12345
    g = _data(rng, (n, Cc, T, H, W))
    modes = [(False, -1), (False, 0), (True, -1)]      # (colour, flip_negate_channel): geometry, optical-flow geometry, colour
    ref = {}
    for colour, neg in modes:
        xin = x if colour else xgeo
        ref[("fwd", colour, neg)] = R.forward_ref(xin, table, colour, neg)
        ref[("bwd", colour, neg)] = R.backward_ref(g if colour else xgeo, table, colour, neg)
    return dict(rows=rows, table=table, x=x, xgeo=xgeo, g=g, modes=modes, ref=ref, n=n)


def _place(a: np.ndarray, layout: str) -> torch.Tensor:
    """The array on the device as a (B, C, T, H, W) view with the layout under test."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if layout == "contiguous":
        return t.to(DEV)
    if layout == "btchw-view":                    # the generators' clips: (B, T, C, H, W) memory viewed as (B, C, T, H, W)
        return t.permute(0, 2, 1, 3, 4).contiguous().to(DEV).permute(0, 2, 1, 3, 4)
    buf = torch.empty(t.numel() + 8, dtype=torch.float32, device=DEV)
    v = buf[1:1 + t.numel()].view(t.shape)        # 4-byte aligned only
    assert v.data_ptr() % 16 == 4
    v.copy_(t)
    return v


class _Guarded:
    """A contiguous output between two NaN bands; `shift` floats off the 16-byte boundary."""

    def __init__(self, shape, shift=0):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * BAND + shift,), float("nan"), dtype=torch.float32, device=DEV)
        self.lo, self.hi = BAND + shift, BAND + shift + n
        self.view = self.buf[self.lo:self.hi].view(shape)

    def intact(self):
        return bool(torch.isnan(self.buf[:self.lo]).all()) and bool(torch.isnan(self.buf[self.hi:]).all())

    def numpy(self):
        return self.view.cpu().numpy()


def _call(name, x, table, y, colour, neg):
    from dcvgan_amd import native
    xd, yd = native.dims5(x), native.dims5(y)
    rc = getattr(_lib(), name)(native.ptr(x), C.byref(xd), native.ptr(table), int(table.shape[0]), native.ptr(y), C.byref(yd), int(colour), int(neg), native.stream_ptr())
    assert rc == 0, (name, rc, _lib().dcv_last_error())


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_apply_and_backward_bit_for_bit(shape, layout):
    from dcvgan_amd import native
    case = _case(shape)
    B = shape[0]
    shift = 1 if layout == "base+4B" else 0
    n0 = native.launch_count()
    worst_rows, checked = [], 0
    for colour, neg in case["modes"]:
        for direction in ("fwd", "bwd"):
            src = case["x"] if colour else case["xgeo"]
            if direction == "bwd" and colour:
                src = case["g"]
            want = case["ref"][(direction, colour, neg)]
            for i in range(0, case["n"], B):
                x = _place(src[i:i + B], layout)
                table = torch.from_numpy(case["table"][i:i + B]).to(DEV)
                out = _Guarded(x.shape, shift)
                _call("dcv_aug_apply" if direction == "fwd" else "dcv_aug_apply_backward", x, table, out.view, colour, neg)
                got = out.numpy()
                assert out.intact(), f"{direction} wrote outside its output ({shape}, {layout}, rows {case['rows'][i:i + B]})"
                same = _bits(got) == _bits(want[i:i + B])
                if not same.all():
                    worst_rows.append((direction, colour, neg, case["rows"][i:i + B], int((~same).sum())))
                checked += got.size
    launches = native.launch_count() - n0
    print(f"\n[augment apply {shape} {layout}] {case['n']} rows x 3 streams x 2 directions: {checked} values, {launches} launches, mismatching batches: {len(worst_rows)}")
    assert not worst_rows, worst_rows[:4]
    # the identity row: bits moved (row 0 of the geometry stream carries -0.0 and a NaN payload)
    y0 = case["ref"][("fwd", False, -1)][0]
    assert np.array_equal(_bits(y0), _bits(case["xgeo"][0])) and _bits(y0)[0, 0, 0, 1] == 0x7FC12345 and _bits(y0)[0, 0, 0, 0] == 0x80000000


def test_backward_into_the_inputs_own_layout():
    """The adjoint's output may be any strided view (a gradient is written in the layout of the tensor it belongs to); the forward's must be contiguous."""
    from dcvgan_amd import native
    shape = (2, 3, 2, 16, 12)
    case = _case((2, 1, 3, 16, 12))
    rng = np.random.default_rng(5)
    g = _data(rng, shape)
    table_np = case["table"][20:22]
    want = R.backward_ref(g, table_np, True, -1)
    table = torch.from_numpy(table_np).to(DEV)
    buf = torch.full((2, 2, 3, 16, 12), float("nan"), dtype=torch.float32, device=DEV)
    out = buf.permute(0, 2, 1, 3, 4)
    _call("dcv_aug_apply_backward", torch.from_numpy(g).to(DEV), table, out, True, -1)
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(want))
    n0 = native.launch_count()
    xd, yd = native.dims5(out), native.dims5(out)
    rc = _lib().dcv_aug_apply(native.ptr(out), C.byref(xd), native.ptr(table), 2, native.ptr(out), C.byref(yd), 1, -1, native.stream_ptr())
    assert rc == native.DCV_EINVAL and native.launch_count() == n0


@pytest.mark.parametrize("shape", [(2, 2, 3, 8, 8), (2, 1, 2, 7, 9), (2, 1, 2, 64, 64)], ids=lambda s: "x".join(map(str, s)))
def test_fan_in_adjoint_bit_for_bit(shape):
    """dcv_aug_fan_backward: ((base + A^T dy0) + A^T dy1) + A^T embed(dyf) in that order; under identity rows it is ops.fan_out's sum, bit for bit."""
    from dcvgan_amd import native, ops
    B, Cc, T, H, W = shape
    rng = np.random.default_rng(11)
    rows = R._rows(H, W)
    rows += [dict()] * (-len(rows) % B)
    table_np = R.make_table(rows)
    frame, bad, launches = T - 1, [], 0
    combos = [(True, 2, True), (True, 1, True), (False, 2, False), (True, 1, False), (False, 1, True)]      # (base, whole cotangents, frame cotangent)
    for i in range(0, len(rows), B):
        tnp = table_np[i:i + B]
        table = torch.from_numpy(tnp).to(DEV)
        base, d0, d1 = (_data(rng, shape) for _ in range(3))
        df = _data(rng, (B, Cc, H, W))
        for has_base, nfull, has_frame in combos:
            want = R.fan_backward_ref(base if has_base else None, [d0, d1][:nfull], df if has_frame else None, frame, tnp, False, 0)
            # the base in the generators' layout, the output in it too
            tb = _place(base, "btchw-view") if has_base else None
            t0, t1 = torch.from_numpy(d0).to(DEV), (torch.from_numpy(d1).to(DEV) if nfull > 1 else None)
            tf = torch.from_numpy(df).to(DEV).unsqueeze(2) if has_frame else None
            out_buf = torch.full((B, T, Cc, H, W), float("nan"), dtype=torch.float32, device=DEV)
            out = out_buf.permute(0, 2, 1, 3, 4)
            dd = lambda t: (native.ptr(t), C.byref(native.dims5(t))) if t is not None else (None, None)
            od = native.dims5(out)
            n0 = native.launch_count()
            rc = _lib().dcv_aug_fan_backward(*dd(tb), *dd(t0), *dd(t1), *dd(tf), frame, native.ptr(table), B, native.ptr(out), C.byref(od), 0, 0, native.stream_ptr())
            assert rc == 0, _lib().dcv_last_error()
            launches += native.launch_count() - n0
            if not np.array_equal(_bits(out.cpu().numpy()), _bits(want)):
                bad.append((rows[i:i + B], has_base, nfull, has_frame))
    # identity rows against the un-augmented fan-in itself
    x = _place(_data(rng, shape), "btchw-view").requires_grad_(True)
    gs = [torch.from_numpy(_data(rng, (B, Cc, H, W))).to(DEV)] + [torch.from_numpy(_data(rng, shape)).to(DEV) for _ in range(3)]
    outs = ops.fan_out(x, frame, 3)
    (want_t,) = torch.autograd.grad(outs, [x], gs)
    ident = torch.from_numpy(R.make_table([dict()] * B)).to(DEV)
    got = torch.empty_strided(x.shape, x.stride(), dtype=torch.float32, device=DEV)
    dd = lambda t: (native.ptr(t), C.byref(native.dims5(t)))
    od = native.dims5(got)
    assert _lib().dcv_aug_fan_backward(*dd(gs[1]), *dd(gs[2]), *dd(gs[3]), *dd(gs[0].unsqueeze(2)), frame, native.ptr(ident), B, native.ptr(got), C.byref(od), 0, -1,
                                       native.stream_ptr()) == 0
    print(f"\n[augment fan-in {shape}] {len(rows)} rows x {len(combos)} operand sets, {launches} launches (one each), mismatches {len(bad)}")
    assert launches == (len(rows) // B) * len(combos)
    assert not bad, bad[:4]
    assert torch.equal(got.view(torch.int32), want_t.view(torch.int32)), "under the identity the fused fan-in is not ops.fan_out's sum"


def test_refusals_launch_nothing():
    from dcvgan_amd import augment, native
    from dcvgan_amd.configs import CONFIGS
    _lib()
    aug = augment.ClipAugment(CONFIGS["debug-isogd-depth"], DEV, p=1.0, adaptive=False, seed=3)
    xg, xc = torch.zeros(2, 1, 2, 8, 8, device=DEV), torch.zeros(2, 3, 2, 8, 8, device=DEV)
    table3 = torch.from_numpy(R.make_table([dict()] * 3)).to(DEV)
    n0, draws = native.launch_count(), aug.rng._counter
    cases = [lambda: aug(xg, xc, table=table3),                                     # a batch that differs from the table's
             lambda: augment.apply(xg, table3, False),
             lambda: augment.apply_backward(xc, table3, True),
             lambda: aug(xg.bfloat16(), xc),                                        # a 16-bit tensor
             lambda: aug(xg, xc.half()),
             lambda: aug(xg.cpu(), xc),                                             # a CPU tensor
             lambda: aug(xg, xc[:, :, :1]),                                         # a pair whose clips differ
             lambda: aug(torch.zeros(1, 1, 1, 2, 4100, device=DEV), torch.zeros(1, 3, 1, 2, 4100, device=DEV))]      # W above the kernel's limit
    n1 = native.launch_count()      # (torch's own casts above launch nothing through the library)
    for k, c in enumerate(cases):
        with pytest.raises(native.NativeError):
            c()
        assert native.launch_count() == n1, k
    assert n1 == n0 and aug.rng._counter == draws, "a refused call drew a table"
    from dcvgan_amd.native import dims5, ptr, stream_ptr
    xd = dims5(xg)
    assert _lib().dcv_aug_apply(ptr(xg), C.byref(xd), ptr(table3), 3, ptr(xg), C.byref(xd), 0, -1, stream_ptr()) == native.DCV_EINVAL
    assert native.launch_count() == n1


# ---- the table ----------------------------------------------------------------------------------------------------------------------------------------------
LIMITS = dict(mx=8, my=8, size=32, contrast=0.5, brightness=1.0, mask=15)
SENTINEL = -77


def _state(p, sum_sign=0, count=0, adjusts=0):
    return torch.tensor([R.f32_bits(p), sum_sign, count, adjusts, 0, 0, 0, 0], dtype=torch.int32).to(DEV)


def _draw(B, H, W, state, seed, offset, lim=LIMITS):
    from dcvgan_amd import native
    buf = torch.full((B * 8 + 2 * BAND,), SENTINEL, dtype=torch.int32, device=DEV)
    table = buf[BAND:BAND + B * 8].view(B, 8)
    l = native.AugLimits(lim["mx"], lim["my"], lim["size"], lim["mask"], lim["contrast"], lim["brightness"])
    rc = _lib().dcv_aug_draw(native.ptr(table), B, H, W, native.ptr(state), C.byref(l), seed, offset, native.stream_ptr())
    assert rc == 0, _lib().dcv_last_error()
    out = table.cpu().numpy()
    assert bool((buf[:BAND] == SENTINEL).all()) and bool((buf[BAND + B * 8:] == SENTINEL).all()), "the draw wrote outside its table"
    return out


def _draw_ref(B, H, W, p, seed, offset, lim=LIMITS):
    return R.draw_ref(B, H, W, p, lim["mx"], lim["my"], lim["size"], lim["contrast"], lim["brightness"], lim["mask"], seed, offset)


@pytest.mark.parametrize("B", [1, 5, 4096])
def test_draw_bit_for_bit(B):
    H = W = 64
    pairs = [(1234, 1), (0xDEADBEEF12345678, (1 << 32) + 5)]
    for seed, offset in pairs:
        for p in (0.0, 0.5, 1.0):
            got = _draw(B, H, W, _state(p), seed, offset)
            want, gates = _draw_ref(B, H, W, p, seed, offset)
            assert np.array_equal(got, want), (B, seed, offset, p, int((got != want).any(1).sum()))
            if p == 0.0:
                assert all(tuple(int(v) for v in r) == R.IDENTITY_ROW for r in got)
            if p == 1.0:
                assert all(bool(g.all()) for g in gates)
                gain, bias = got[:, 6].copy().view(F32), got[:, 7].copy().view(F32)
                assert np.abs(got[:, 1]).max() <= 8 and np.abs(got[:, 2]).max() <= 8 and set(got[:, 5].tolist()) == {32}
                assert got[:, 3].min() >= -16 and got[:, 3].max() <= 47 and got[:, 4].min() >= -16 and got[:, 4].max() <= 47
                assert 0.5 < gain.min() and gain.max() <= 1.5 and -0.5 < bias.min() and bias.max() <= 0.5
    a, b, c = _draw(B, H, W, _state(1.0), 1234, 1), _draw(B, H, W, _state(1.0), 1234, 1), _draw(B, H, W, _state(1.0), 1234, 2)
    assert np.array_equal(a, b) and not np.array_equal(a, c)      # the same (seed, offset): the same bits; the next offset: another table
    print(f"\n[augment draw B = {B}] 2 (seed, offset) pairs x 3 probabilities equal the restatement bit for bit")


def test_draw_gate_frequencies_and_p_from_the_state_block():
    B, H, W = 4096, 64, 64
    got = _draw(B, H, W, _state(0.5), 1234, 1)
    want, gates = _draw_ref(B, H, W, 0.5, 1234, 1)
    assert np.array_equal(got, want)
    counts = [int(g.sum()) for g in gates]      # (the gates themselves are not in the table; the table equals the restatement's, whose gates these are)
    flips = int(got[:, 0].sum())
    print(f"\n[augment draw frequencies] gates on {counts} of {B} (2048 +- 160), flips {flips} (1024 +- 139)")
    assert all(abs(c - 2048) <= 160 for c in counts) and abs(flips - 1024) <= 139
    # p is read on the device: change word 0 between two draws and the second table follows it
    state = _state(0.0)
    t0 = _draw(64, H, W, state, 7, 1)
    state.copy_(torch.tensor([R.f32_bits(1.0), 0, 0, 0, 0, 0, 0, 0], dtype=torch.int32))
    t1 = _draw(64, H, W, state, 7, 1)
    assert all(tuple(int(v) for v in r) == R.IDENTITY_ROW for r in t0)
    assert np.array_equal(t1, _draw_ref(64, H, W, 1.0, 7, 1)[0]) and set(t1[:, 5].tolist()) == {32}
    # a disabled op writes its identity words
    lim = dict(LIMITS, mask=R.FLIP | R.CUTOUT)
    t2 = _draw(64, H, W, _state(1.0), 7, 1, lim)
    assert np.array_equal(t2, _draw_ref(64, H, W, 1.0, 7, 1, lim)[0]) and not t2[:, 1].any() and set(t2[:, 6].tolist()) == {R.ONE_BITS}


# ---- the adaptive probability ---------------------------------------------------------------------------------------------------------------------------------
def test_observe_and_adjust_follow_the_rule():
    from dcvgan_amd import native
    L = _lib()
    nan = float("nan")
    target, step, p_max = 0.6, 0.25, 0.4
    # 6 adjustments: clamp at 0; up; clamp at p_max; count == 0; r == target exactly; down
    rounds = [[[1.0, 2.0, -1.0, 0.0, nan]], [[1.0] * 4, [0.5, 3.0]], [[1.0] * 300 + [-0.0]], [], [[1.0, 1.0, 1.0, 1.0, -1.0]], [[-1.0, -2.0], [0.0, nan, 1.0]]]
    state, want = _state(0.0), [R.f32_bits(0.0), 0, 0, 0, 0, 0, 0, 0]
    ps = []
    for logits in rounds:
        for y in logits:
            buf = torch.full((len(y) + 2 * BAND,), nan, dtype=torch.float32, device=DEV)
            buf[BAND:BAND + len(y)] = torch.tensor(y, dtype=torch.float32)
            assert L.dcv_aug_observe(native.ptr(buf[BAND:]), len(y), native.ptr(state), native.stream_ptr()) == 0
            want = R.observe_ref(want, y)
            assert state.cpu().tolist() == want, (state.cpu().tolist(), want)
        assert L.dcv_aug_adjust(native.ptr(state), target, step, p_max, native.stream_ptr()) == 0
        want = R.adjust_ref(want, target, step, p_max)
        got = state.cpu().tolist()
        assert got == want, (got, want)
        assert got[1] == 0 and got[2] == 0 and got[4:] == [0, 0, 0, 0]
        ps.append(float(R.bits_f32(got[0])))
    print(f"\n[augment adjust] p over 6 adjustments: {ps}; adjusts = {want[3]}")
    assert ps == [0.0, 0.25, float(F32(0.4)), float(F32(0.4)), float(F32(0.4)), float(F32(0.4) - F32(0.25))] and want[3] == 6


# ---- the module -----------------------------------------------------------------------------------------------------------------------------------------------
def _cfg(name="debug-isogd-depth"):
    from dcvgan_amd.configs import CONFIGS
    return CONFIGS[name]


def test_module_under_autograd():
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    from dcvgan_amd import augment, native
    _lib()
    rng = np.random.default_rng(2)
    aug = augment.ClipAugment(_cfg("isogd-flow"), DEV, p=1.0, adaptive=False, seed=77)
    assert aug.neg_g == 0 and aug.neg_c == -1
    xg_np, xc_np = _data(rng, (2, 2, 2, 16, 16)), _data(rng, (2, 3, 2, 16, 16))
    gg_np, gc_np = _data(rng, (2, 2, 2, 16, 16)), _data(rng, (2, 3, 2, 16, 16))
    xg, xc = _place(xg_np, "btchw-view").requires_grad_(True), _place(xc_np, "btchw-view").requires_grad_(True)
    gg, gc = torch.from_numpy(gg_np).to(DEV), torch.from_numpy(gc_np).to(DEV)
    torch.cuda.synchronize()
    n0, m0 = native.launch_count(), augment.launches()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        torch.cuda.set_sync_debug_mode("error")      # (inside the profiler's own start / stop, which synchronise)
        try:
            yg, yc = aug(xg, xc)
            n1 = native.launch_count()
            dg, dc = torch.autograd.grad([yg, yc], [xg, xc], [gg, gc])
            n2 = native.launch_count()
            yg2, yc2 = aug(xg, xc)
            (dc_only,) = torch.autograd.grad([yc2], [xc], [gc])      # the geometry stream's cotangent is None: its adjoint is skipped
            n3 = native.launch_count()
            with torch.no_grad():
                aug(xg, xc)                                              # nothing asks for a gradient: no tape entry
            plain = aug(xg.detach(), xc.detach())
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
    kernels = {e.key: e.count for e in prof.key_averages() if e.device_type == DeviceType.CUDA}
    foreign = {k[:160]: n for k, n in kernels.items() if "at::" in k or "torch" in k.lower()}
    assert not foreign, foreign
    assert any("aug_rows_kernel" in k for k in kernels) and any("aug_draw_kernel" in k for k in kernels), sorted(kernels)
    print(f"\n[augment module] launches: forward {n1 - n0} (1 draw + 2 applies), backward {n2 - n1}, second pair with one cotangent {n3 - n2} (3 + 1); kernels {sorted(k[:40] for k in kernels)}")
    assert (n1 - n0, n2 - n1, n3 - n2) == (3, 2, 4)
    assert augment.launches() - m0 == native.launch_count() - n0      # the module's own count (what the iteration tests hold the formula against) is the library's
    assert plain[0].grad_fn is None and not plain[0].requires_grad
    # the tables the module drew: offsets 1 and 2 of its own stream, key = seed + SEED_SALT
    lim = aug.limits(16, 16)
    seed = (77 + augment.SEED_SALT) & 0xFFFFFFFFFFFFFFFF
    t1 = R.draw_ref(2, 16, 16, 1.0, lim.mx, lim.my, lim.size, lim.contrast, lim.brightness, lim.mask, seed, 1)[0]
    t2 = R.draw_ref(2, 16, 16, 1.0, lim.mx, lim.my, lim.size, lim.contrast, lim.brightness, lim.mask, seed, 2)[0]
    assert (lim.mx, lim.my, lim.size) == (2, 2, 8)
    for got, want in [(yg, R.forward_ref(xg_np, t1, False, 0)), (yc, R.forward_ref(xc_np, t1, True, -1)), (dg, R.backward_ref(gg_np, t1, False, 0)),
                      (dc, R.backward_ref(gc_np, t1, True, -1)), (yc2, R.forward_ref(xc_np, t2, True, -1)), (dc_only, R.backward_ref(gc_np, t2, True, -1))]:
        assert np.array_equal(_bits(got.detach().cpu().numpy()), _bits(want))
    assert yg.is_contiguous() and dg.stride() == xg.stride() and dc.stride() == xc.stride()      # gradients in their tensors' own layout
    # an injected table draws nothing
    c0, n4 = aug.rng._counter, native.launch_count()
    inj = torch.from_numpy(R.make_table([dict(flip=1), dict(dx=2, cs=4)])).to(DEV)
    yi = aug(xg.detach(), xc.detach(), table=inj)
    assert aug.rng._counter == c0 and native.launch_count() - n4 == 2
    assert np.array_equal(_bits(yi[0].cpu().numpy()), _bits(R.forward_ref(xg_np, inj.cpu().numpy(), False, 0)))


def test_state_dict_round_trip():
    from dcvgan_amd import augment
    _lib()
    a = augment.ClipAugment(_cfg(), DEV, p=0.7, adaptive=True, interval=3, seed=5)
    a.draw(4, 64, 64)
    a.observe(torch.tensor([1.0, -2.0, 3.0], device=DEV))
    sd = a.state_dict()
    nxt = [a.draw(4, 64, 64).cpu(), a.draw(4, 64, 64).cpu()]
    b = augment.ClipAugment(_cfg(), DEV, p=0.1, adaptive=False, interval=9, seed=123)
    b.load_state_dict(sd)
    got = [b.draw(4, 64, 64).cpu(), b.draw(4, 64, 64).cpu()]
    assert all(torch.equal(x, y) for x, y in zip(nxt, got)) and not torch.equal(nxt[0], nxt[1])
    assert b.state_words() == sd["state"] and sd["state"][1:3] == [1, 3] and b.adaptive and b.interval == 3 and abs(b.p() - 0.7) < 1e-7
    print(f"\n[augment state_dict] state {sd['state']}, rng {sd['rng']}: the next two tables are bit-identical after the round trip")


# ---- the iteration --------------------------------------------------------------------------------------------------------------------------------------------
def _iterate(iters, aug_kw, cfg_name="debug-isogd-depth", seed=21):
    from dcvgan_amd import native, trainer
    native.lib()
    cfg = _cfg(cfg_name).scaled(batchsize=2)
    models, r = rig.seeded_models(cfg, DEV, seed, 9)
    xc, xg = rig.clip_pair(cfg, DEV, 4)
    opts = trainer.build_optimizers(cfg, models)
    aug = trainer.build_augment(cfg, models, opts, **aug_kw) if aug_kw is not None else None
    runner = trainer.StepRunner(cfg, models, opts, trainer.build_loss(cfg), sync_losses=True, augment=aug)
    from dcvgan_amd import augment
    losses, launches, own, grads = [], [], [], None
    for it in range(iters):
        n0, m0 = native.launch_count(), augment.launches()
        losses.append(runner.step(xc, xg, 2 + it))
        launches.append(native.launch_count() - n0)
        own.append(augment.launches() - m0)
        if it == 0:
            grads = {n: {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in models[n].named_parameters()} for n in ("ggen", "cgen")}
    torch.cuda.synchronize()
    state = {n: {k: v.detach().clone() for k, v in m.state_dict().items()} for n, m in models.items()}
    return dict(cfg=cfg, losses=losses, launches=launches, own=own, state=state, grads=grads, aug=aug, model_draws=r._counter)


def _same_state(a, b):
    return all(torch.equal(a[n][k].reshape(-1).view(torch.uint8), b[n][k].reshape(-1).view(torch.uint8)) for n in a for k in a[n])


@pytest.fixture(scope="module")
def runs():
    return dict(none=_iterate(2, None), p0=_iterate(2, dict(adaptive=False, p=0.0, seed=31)), p1a=_iterate(2, dict(adaptive=False, p=1.0, seed=31)),
                p1b=_iterate(2, dict(adaptive=False, p=1.0, seed=31)))


def test_iteration_at_p0_is_the_iteration_without_augmentation(runs):
    none, p0 = runs["none"], runs["p0"]
    print(f"\n[augment iteration p = 0] losses {p0['losses'][1]} vs {none['losses'][1]}; launches {p0['launches']} vs {none['launches']}")
    assert p0["losses"] == none["losses"]                               # every loss, as Python floats: equal bits
    assert _same_state(p0["state"], none["state"])                      # every parameter and BatchNorm buffer
    assert p0["model_draws"] == none["model_draws"]                     # the models' random streams are untouched
    assert p0["aug"].draws == 6


def test_iteration_at_p1(runs):
    none, p0, a, b = runs["none"], runs["p0"], runs["p1a"], runs["p1b"]
    print(f"\n[augment iteration p = 1] losses {a['losses'][1]}; launches {a['launches']} vs {none['launches']} without")
    assert a["losses"] == b["losses"] and _same_state(a["state"], b["state"])      # two runs: the same bits
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
    # launches the augmentation issues per iteration (both phases of this config carry a tape and run their backward): the formula, nothing else
    aug = a["aug"]
    assert none["own"] == [0, 0]
    for it in (1, 2):
        formula = aug.launches_per_iteration(it, taped_phases=2)
        assert formula == 3 + 6 + 2 * 2
        assert a["own"][it - 1] == formula and p0["own"][it - 1] == formula, (a["own"], p0["own"])
        assert p0["launches"][it - 1] == a["launches"][it - 1]      # the table's values change no launch


def test_iteration_adaptive():
    run = _iterate(4, dict(adaptive=True, p=0.0, interval=2, adjust_clips=8, seed=31))
    aug = run["aug"]
    words = aug.state_words()
    step = F32(2 * 2 / 8)
    reachable = {float(min(max(F32(k) * step, F32(0.0)), F32(0.8))) for k in range(0, 3)}
    print(f"\n[augment iteration adaptive] state {words}, p = {aug.p()}, reachable {sorted(reachable)}; launches {run['launches']}, the augmentation's own {run['own']}")
    assert aug.adjusts() == 2 and words[1:3] == [0, 0] and words[4:] == [0, 0, 0, 0]
    assert aug.p() in reachable
    for it in range(1, 5):
        assert aug.launches_per_iteration(it, 2) == 3 + 6 + 4 + 3 + (1 if it % 2 == 0 else 0)
        assert run["own"][it - 1] == aug.launches_per_iteration(it, 2), run["own"]


def test_optical_flow_wiring():
    from dcvgan_amd import trainer
    run = _iterate(1, dict(adaptive=False, p=1.0, seed=8), cfg_name="isogd-flow")
    aug = run["aug"]
    assert (aug.neg_g, aug.neg_c) == (0, -1) and all(math.isfinite(v) for v in run["losses"][0].values())
    assert trainer.build_augment(_cfg(), {"idis": torch.nn.Linear(1, 1).to(DEV)}, None, adaptive=False).neg_g == -1
