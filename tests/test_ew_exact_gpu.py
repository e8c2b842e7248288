"""GPU: the fp32 elementwise dispatcher, the device RNG, the GAN losses, the GRU recurrence, the channel softmax / argmax entries and the flow visualisation
against the host references of tests/exactew.py — bit for bit where that module proves it possible, within a counted bound elsewhere.  Every entry is called
through the C ABI on views the test lays out itself; every output sits between two 8192-element guard bands (NaN, or the byte 0xA5) that must survive, and no
NaN may appear inside a view.  No expected value comes from the device, with one exception: dcv_noise_add is compared with dcv_normal_fill of the same stream,
which this file compares with the host Philox / Box-Muller restatement.

Each dispatcher case asserts, from tests/exactbn.py's copy of the dispatch arithmetic, the kernel it is meant to reach (ew_rows, ew<4>, ew<1> over a contiguous
plane, ew<1> with inner == 1), so it cannot move to another one unnoticed."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

from tests import exactbn as X
from tests import exactew as E
from tests import rig

pytestmark = pytest.mark.gpu
NOTES = {"normal_fill_max_err": 0.0, "cl_noise_max_err": 0.0, "gru": {}}
G = X.GUARD
TANH_ULPS = 5          # tests/test_bn_exact_gpu.py: OpenCL C "relative error as ULPs", tanh <= 5 ulp
BYTE = 0xA5


@pytest.fixture(scope="module")
def dev():
    from dcvgan_amd import native
    native.lib()
    yield torch.device("cuda:0")
    out = os.environ.get("DCV_EW_NOTES_OUT")      # a measuring run keeps the observed figures (tests/golden/ew_exact_notes.json records them)
    if out:
        with open(out, "w") as f:
            json.dump(NOTES, f, indent=1)


@pytest.fixture(autouse=True)
def _stop_after_fault():
    """After a device fault (seen here or anywhere else through tests/rig.py) nothing else of this module is started on the GPU"""
    rig.stop_after_fault()
    yield


sync = rig.sync


def call(name, *args):
    from dcvgan_amd import native as N
    L = N.lib()
    rc = getattr(L, name)(*args)
    assert rc == N.DCV_OK, (name, rc, L.dcv_last_error())


def P(t):
    from dcvgan_amd import native as N
    return N.ptr(t)


def D(t):
    from dcvgan_amd import native as N
    return C.byref(N.dims5(t))


def S():
    from dcvgan_amd import native as N
    return N.stream_ptr()


def f32(values):
    return torch.from_numpy(np.asarray(values, dtype=np.float32))


def bits_equal(a, b):
    it = {4: torch.int32, 2: torch.int16, 1: torch.uint8}[a.element_size()]
    return bool(torch.equal(a.contiguous().view(it), b.contiguous().view(it)))


# ---- guarded operands --------------------------------------------------------------------------------------------------------------------------------------
def g_in(shape, layout, dev, fill):
    return X.guarded(shape, layout, dev, fill=fill.float())[0]


class Out:
    """An output view of `shape` in `layout` inside a NaN-guarded, NaN-filled allocation"""

    def __init__(self, shape, layout, dev):
        self.shape, self.layout = shape, layout
        self.view, self.storage = X.guarded(shape, layout, dev)
        self.before = self.storage.clone()

    def check(self, what, want, bound=None, owner=None):
        """No NaN inside, nothing outside touched, and the values: bit for bit against fp64 rounded to fp32 where `bound` is None"""
        sync()
        got = self.view.detach().cpu()
        assert not bool(torch.isnan(got).any()), f"{what}: NaN inside the view (an element not written, or read from outside an operand)"
        assert X.untouched_outside(self.storage, self.before, self.shape, self.layout), f"{what}: written outside the output view"
        r = X.assert_within(what, got, want, 0.0 if bound is None else bound, self.shape, owner)
        if bound is None:
            assert bits_equal(got, want.float()), f"{what}: equal in value but not in bits (a signed zero)"
        return r


class Flat:
    """n elements between two guard bands of G elements: NaN for floating types, the byte 0xA5 for uint8"""

    def __init__(self, n, dev, dtype=torch.float32, fill=None):
        self.n, self.u8 = n, dtype == torch.uint8
        self.buf = torch.full((n + 2 * G,), BYTE if self.u8 else float("nan"), dtype=dtype, device=dev)
        self.v = self.buf[G:G + n]
        if fill is not None:
            self.v.copy_(torch.as_tensor(fill).to(dtype))

    def intact(self):
        lo, hi = self.buf[:G], self.buf[G + self.n:]
        if self.u8:
            return bool((lo == BYTE).all()) and bool((hi == BYTE).all())
        return bool(torch.isnan(lo.float()).all()) and bool(torch.isnan(hi.float()).all())

    def get(self, what):
        sync()
        assert self.intact(), f"{what}: a guard band was written"
        got = self.v.detach().cpu()
        if not self.u8:
            assert not bool(torch.isnan(got.float()).any()), f"{what}: NaN inside (an element not written, or read from outside an operand)"
        return got


def act_code(act):
    from dcvgan_amd import native as N
    return {"leaky": N.ACT_LEAKY, "none": N.ACT_NONE, "tanh": N.ACT_TANH}[act]


@functools.lru_cache(maxsize=2)
def ew_operands(name):
    return E.ew_operands(name, E.ew_case(name).shape)


def lays_for(case, combo, k):
    lays = E.operand_layouts(combo, k)
    path, d = E.ew_path(case.shape, lays)
    assert path == case.path, f"{case.name} {lays}: the dispatcher takes {path}, the case is meant for {case.path}"
    return lays, d


EW_IDS = [f"{n}-{i}" for n, i in E.EW_PARAMS]


# ---- 1. the fp32 elementwise dispatcher --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,ci", E.EW_PARAMS, ids=EW_IDS)
def test_activations_and_axpby(dev, name, ci):
    case = E.ew_case(name)
    combo, shape = case.combos[ci], case.shape
    o = ew_operands(name)
    own = lambda d: (lambda idx: X.owner32(d, shape, idx))
    for act in (("leaky",) if case.big else ("leaky", "none", "tanh")):
        (lx, ly), d = lays_for(case, combo, 2)
        x, y = g_in(shape, lx, dev, o["x"] / (16.0 if act == "tanh" else 1.0)), Out(shape, ly, dev)
        call("dcv_act_forward", P(x), D(x), P(y.view), D(y.view), act_code(act), E.SLOPE, S())
        want = E.act_forward_ref(o["x"] / (16.0 if act == "tanh" else 1.0), act)
        y.check(f"act_forward {act} {case.path}", want, TANH_ULPS * 2 * E.U * want.abs() if act == "tanh" else None, own(d))
    if case.big:
        return
    for act, yk in (("leaky", "yl"), ("tanh", "yt"), ("none", "yl")):
        (l0, l1, l2), d = lays_for(case, combo, 3)
        dy, yy, dx = g_in(shape, l0, dev, o["dy"]), g_in(shape, l1, dev, o[yk]), Out(shape, l2, dev)
        call("dcv_act_backward", P(dy), D(dy), P(yy), D(yy), P(dx.view), D(dx.view), act_code(act), E.SLOPE, S())
        dx.check(f"act_backward {act} {case.path}", E.act_backward_ref(o["dy"], o[yk], act), None, own(d))
    (l0, l1, l2), d = lays_for(case, combo, 3)
    x, z, y = g_in(shape, l0, dev, o["x"]), g_in(shape, l1, dev, o["z"]), Out(shape, l2, dev)
    call("dcv_axpby", P(x), D(x), E.AXPBY_A, P(z), D(z), E.AXPBY_B, P(y.view), D(y.view), S())
    y.check(f"axpby with z {case.path}", E.axpby_ref(o["x"], o["z"]), None, own(d))
    (l0, l2), d = lays_for(case, combo, 2)
    x, y = g_in(shape, l0, dev, o["x"]), Out(shape, l2, dev)
    call("dcv_axpby", P(x), D(x), E.AXPBY_A, None, None, 0.0, P(y.view), D(y.view), S())
    y.check(f"axpby without z {case.path}", E.axpby_ref(o["x"]), None, own(d))


@pytest.mark.parametrize("name,ci", [p for p in E.EW_PARAMS if not E.ew_case(p[0]).big], ids=[i for p, i in zip(E.EW_PARAMS, EW_IDS) if not E.ew_case(p[0]).big])
def test_videos_to_uint8(dev, name, ci):
    case = E.ew_case(name)
    shape = case.shape
    (lx,), d = lays_for(case, case.combos[ci], 1)
    xh = E.u8_operands(name, shape)
    x = X.guarded(shape, lx, dev, fill=torch.from_numpy(xh))[0]
    for rep in (1, 3):
        want = E.to_u8_ref(xh, rep)
        out = Flat(want.size, dev, torch.uint8)
        call("dcv_videos_to_uint8", P(x), D(x), P(out.v), rep, S())
        got = out.get(f"videos_to_uint8 x{rep}").numpy().reshape(want.shape)
        bad = got != want
        assert not bad.any(), f"videos_to_uint8 x{rep} {case.path}: {int(bad.sum())} of {bad.size} bytes differ, first at {tuple(int(v[0]) for v in np.nonzero(bad))}"


# ---- 2. the RNG contract -----------------------------------------------------------------------------------------------------------------------------------
STREAMS = [(E.SEED_HI, E.OFFSET_HI), (1234, 7)]


@pytest.mark.parametrize("p", E.DROPOUT_EXACT_P + E.DROPOUT_ULP_P)
def test_dropout_mask_against_host_philox(dev, p):
    for seed, offset in STREAMS:
        for n in E.RNG_N:
            m = Flat(n, dev)
            call("dcv_dropout_mask", P(m.v), n, p, seed, offset, S())
            got = m.get(f"dropout_mask n {n}")
            want = torch.from_numpy(E.dropout_ref(n, p, seed, offset))
            what = f"dropout_mask p {p} n {n} seed {seed:#x} offset {offset:#x}"
            zero = want == 0
            assert torch.equal(got == 0, zero), f"{what}: the zero pattern differs, first at element {int(((got == 0) != zero).nonzero()[0])}"
            if p in E.DROPOUT_EXACT_P:
                assert bits_equal(got, want), what
            else:
                keep = want.max()
                assert bool(((got[~zero] - keep).abs() <= X.ulp32(keep.double()).float()).all()), what


@pytest.mark.parametrize("n", E.RNG_N)
def test_normal_fill_against_host_box_muller(dev, n):
    for seed, offset in STREAMS:
        z = Flat(n, dev)
        call("dcv_normal_fill", P(z.v), n, seed, offset, S())
        got = z.get(f"normal_fill n {n}").double().numpy()
        ref = E.normal_ref(n, seed, offset)
        err = E.normal_err(got, ref)
        NOTES["normal_fill_max_err"] = max(NOTES["normal_fill_max_err"], err)
        print(f"normal_fill n {n} seed {seed:#x}: max |z - z_ref| / (1 + |z_ref|) = {err:.3e}")
        bad = np.abs(got - ref) > E.NORMAL_CAP * (1 + np.abs(ref))
        assert not bad.any(), f"normal_fill n {n} seed {seed:#x} offset {offset:#x}: {int(bad.sum())} of {n} beyond the cap, first element {int(np.nonzero(bad)[0][0])}: got {got[bad][0]!r}, expected {ref[bad][0]!r}"


@pytest.mark.parametrize("n,count", [(5, 3), (1025, 4), (4, 2), (1, 5)])
def test_normal_fill_many_against_host_box_muller(dev, n, count):
    seed, offset = E.SEED_HI, 2 ** 32 - 2           # offset + j carries into the high word
    z = Flat(n * count, dev)
    call("dcv_normal_fill_many", P(z.v), n, count, seed, offset, S())
    got = z.get("normal_fill_many").double().numpy().reshape(count, n)
    ref = E.normal_many_ref(n, count, seed, offset)
    err = E.normal_err(got, ref)
    NOTES["normal_fill_max_err"] = max(NOTES["normal_fill_max_err"], err)
    bad = np.abs(got - ref) > E.NORMAL_CAP * (1 + np.abs(ref))
    assert not bad.any(), f"normal_fill_many n {n} count {count}: {int(bad.sum())} beyond the cap, first (draw, element) {tuple(int(v[0]) for v in np.nonzero(bad))}"


@pytest.mark.parametrize("name,ci", E.EW_PARAMS, ids=EW_IDS)
def test_noise_add_is_x_plus_sigma_times_the_stream(dev, name, ci):
    case = E.ew_case(name)
    shape = case.shape
    o = ew_operands(name)
    numel = o["x"].numel()
    (lx, ly), d = lays_for(case, case.combos[ci], 2)
    x = g_in(shape, lx, dev, o["x"])
    for sigma, (seed, offset) in zip((0.5, 2.0), STREAMS):
        z = Flat(numel, dev)
        call("dcv_normal_fill", P(z.v), numel, seed, offset, S())      # compared with the host in test_normal_fill_against_host_box_muller
        zh = z.get("normal_fill").double().view(shape)                # element e of the logical (N, C, D, H, W) order
        y = Out(shape, ly, dev)
        call("dcv_noise_add", P(x), D(x), P(y.view), D(y.view), sigma, seed, offset, S())
        # sigma z is exact (a power of two), so x + sigma z rounds once, fused or not
        y.check(f"noise_add sigma {sigma} {case.path}", (o["x"] + sigma * zh).float().double(), None, lambda idx: X.owner32(d, shape, idx))


def cl_storage(shape, dev, dtype, fill=None, body=float("nan")):
    """A channels-last 16-bit tensor of ops_cl.cl_empty's strides inside a guarded allocation -> (view (N, C, D, H, W), whole pixels (N, PIX, pitch), storage)"""
    from dcvgan_amd import ops_cl
    N, Cc, Dd, H, W = shape
    pitch = ops_cl.pitch_of(Cc)
    numel = N * Dd * H * W * pitch
    st = torch.full((numel + 2 * G,), float("nan"), dtype=dtype, device=dev)
    st[G:G + numel] = body
    full = st[G:G + numel].view(N, Dd, H, W, pitch)
    v = full.permute(0, 4, 1, 2, 3)[:, :Cc]
    if fill is not None:
        v.copy_(fill)
    return v, full.view(N, Dd * H * W, pitch), st


def cl_fn(dtype):
    return "dcv_clf16_elementwise" if dtype == torch.float16 else "dcv_cl_elementwise"


def cl_check_padding(what, pix, st, Cc):
    """Channels C .. Cpad - 1 exactly zero, the rest of the pitch and the guard bands as they were (NaN)"""
    sync()
    cpad = (Cc + 7) // 8 * 8
    p = pix.detach().cpu().float()
    assert bool((p[:, :, Cc:cpad] == 0).all()), f"{what}: padding channels are not zero"
    assert bool(torch.isnan(p[:, :, cpad:]).all()), f"{what}: written past the padded channels"
    assert bool(torch.isnan(st[:G].float()).all()) and bool(torch.isnan(st[-G:].float()).all()), f"{what}: a guard band was written"
    assert not bool(torch.isnan(p[:, :, :Cc]).any()), f"{what}: NaN inside"


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("shape", E.CL_NOISE_SHAPES, ids=str)
def test_cl16_noise_against_host_box_muller(dev, shape, dtype):
    from dcvgan_amd import ops_cl
    seed, offset = E.SEED_HI, E.OFFSET_HI
    ref = E.cl_noise_ref(shape, seed, offset)
    Cc = shape[1]
    tol = E.NORMAL_CAP * (1 + np.abs(ref))
    tol = tol + E.half_ulp(np.abs(ref) + tol, dtype)

    def judge(what, y):
        got = y.detach().cpu().double().numpy()
        err = float(np.max(np.maximum(np.abs(got - ref) - E.half_ulp(np.abs(ref), dtype), 0.0) / (1 + np.abs(ref))))
        NOTES["cl_noise_max_err"] = max(NOTES["cl_noise_max_err"], err)
        print(f"{what} {shape} {dtype}: max (|y - z_ref| - half ulp) / (1 + |z_ref|) = {err:.3e}")
        bad = np.abs(got - ref) > tol
        assert not bad.any(), f"{what} {shape} {dtype}: {int(bad.sum())} of {bad.size} beyond the cap, first at {tuple(int(v[0]) for v in np.nonzero(bad))}"

    # through the C entry, into guarded storage
    x, _, _ = cl_storage(shape, dev, dtype, body=0.0)
    y, ypix, yst = cl_storage(shape, dev, dtype)
    call(cl_fn(dtype), 2, P(x), D(x), None, None, P(y), D(y), 1.0, 0.0, seed, offset, S())
    cl_check_padding("cl noise", ypix, yst, Cc)
    judge("cl_elementwise kind 2", y)
    # and through ops_cl.noise_add, the call the models make
    ops_cl.enable(False, half="fp16" if dtype == torch.float16 else "bf16")
    try:
        x2 = ops_cl.cl_empty(shape, dev, zero=True)
        y2 = ops_cl.noise_add(x2, 1.0, None, seed, offset)
        sync()
    finally:
        ops_cl.enable(False, half="bf16")
    assert y2.dtype == dtype and bits_equal(y2.detach().cpu(), y.detach().cpu())
    cpad, pitch = (Cc + 7) // 8 * 8, ops_cl.pitch_of(Cc)
    whole = torch.as_strided(y2, (shape[0], shape[2] * shape[3] * shape[4], pitch), (shape[2] * shape[3] * shape[4] * pitch, pitch, 1), y2.storage_offset())
    assert bool((whole[:, :, Cc:cpad].float() == 0).all())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("shape", E.CL_NOISE_SHAPES, ids=str)
def test_cl16_elementwise_kinds_in_small_integers(dev, shape, dtype):
    g = torch.Generator().manual_seed(X.seed_of(f"cl-ew:{shape}"))
    a = torch.randint(-8, 9, shape, generator=g).double()
    b = torch.randint(-3, 4, shape, generator=g).double()
    cases = {0: (a, None, 0.0, 0.0, a),
             1: (a, b, 2.0, -3.0, 2.0 * a - 3.0 * b),
             3: (a, b, 0.25, 0.0, a * torch.where(b > 0, 1.0, 0.25)),
             4: (a, b, 0.0, 0.0, a * (1.0 - b * b)),
             5: (a, None, 0.25, 0.0, torch.where(a > 0, a, a * 0.25))}
    for kind, (xh, zh, ca, cb, want) in cases.items():
        assert bool((want.to(dtype).double() == want).all())           # exact in the 16-bit type
        x, _, _ = cl_storage(shape, dev, dtype, fill=xh.to(dtype), body=0.0)
        z = cl_storage(shape, dev, dtype, fill=zh.to(dtype), body=0.0)[0] if zh is not None else None
        y, ypix, yst = cl_storage(shape, dev, dtype)
        call(cl_fn(dtype), kind, P(x), D(x), P(z), D(z) if z is not None else None, P(y), D(y), ca, cb, 0, 0, S())
        cl_check_padding(f"cl_elementwise kind {kind}", ypix, yst, shape[1])
        got = y.detach().cpu()
        assert bits_equal(got, want.to(dtype)), f"cl_elementwise kind {kind} {shape} {dtype}: " + X.first_mismatch(got.double() != want, got.double(), want, shape, None)


# ---- 3. GAN losses -----------------------------------------------------------------------------------------------------------------------------------------
def run_loss(dev, yh, kind, accumulate=0, preset=None, with_dy=True):
    n = len(yh)
    y = Flat(n, dev, fill=torch.from_numpy(yh))
    loss = Flat(1, dev, fill=[0.0 if preset is None else preset])
    dy = Flat(n, dev) if with_dy else None
    call("dcv_gan_loss", P(y.v), n, kind, P(loss.v), accumulate, P(dy.v) if with_dy else None, S())
    lv = loss.get("gan_loss value")
    return lv, (dy.get("gan_loss dy") if with_dy else None)


@pytest.mark.parametrize("kind", E.HINGE_KINDS)
@pytest.mark.parametrize("n", E.LOSS_N)
def test_hinge_losses_bit_for_bit(dev, n, kind):
    yh = E.loss_logits(n, kind)
    want_l, want_dy = E.hinge_expected(yh, kind)
    lv, dy = run_loss(dev, yh, kind)
    assert bits_equal(lv, f32([want_l])), f"hinge kind {kind} n {n}: loss {float(lv)!r}, expected {float(want_l)!r}"
    wd = torch.from_numpy(want_dy)
    assert bits_equal(dy, wd), f"hinge kind {kind} n {n}: " + X.first_mismatch(dy != wd, dy.double(), wd.double(), (n,), None)
    acc, _ = run_loss(dev, yh, kind, accumulate=1, preset=3.25)
    assert bits_equal(acc, f32([np.float32(3.25) + want_l])), f"accumulate: {float(acc)!r}"
    nody, none = run_loss(dev, yh, kind, with_dy=False)
    assert none is None and bits_equal(nody, f32([want_l]))


@pytest.mark.parametrize("kind", E.SOFTPLUS_KINDS)
@pytest.mark.parametrize("n", E.LOSS_N)
def test_softplus_losses_within_the_counted_bound(dev, n, kind):
    yh = E.loss_logits(n, kind)
    loss, bl, dyr, bdy = E.softplus_bounds(yh, kind)
    lv, dy = run_loss(dev, yh, kind)
    got_l, got_dy = float(lv.double()), dy.double().numpy()
    assert np.isfinite(got_l) and np.isfinite(got_dy).all()
    print(f"softplus kind {kind} n {n}: loss error / bound {abs(got_l - loss) / bl:.3f}, worst dy error / bound {float(np.max(np.abs(got_dy - dyr) / bdy)):.3f}")
    assert abs(got_l - loss) <= bl, f"kind {kind} n {n}: loss {got_l!r}, expected {loss!r}, bound {bl!r}"
    bad = np.abs(got_dy - dyr) > bdy
    assert not bad.any(), f"kind {kind} n {n}: dy beyond its bound at element {int(np.nonzero(bad)[0][0])} (logit {yh[bad][0]!r}): got {got_dy[bad][0]!r}, expected {dyr[bad][0]!r}"
    inv = float(E.inv32(n))
    for v, g_at in ((100.0, 0.0 if kind != 1 else inv), (-100.0, -inv if kind != 1 else 0.0)):      # expf overflows or vanishes: exactly 0 or -+1/n
        at = yh == v
        assert bool((got_dy[at] == g_at).all()), f"kind {kind} n {n}: gradient at {v} is {got_dy[at]!r}, expected exactly {g_at!r}"
    acc, _ = run_loss(dev, yh, kind, accumulate=1, preset=3.25)
    assert abs(float(acc.double()) - (3.25 + loss)) <= bl + E.U * (3.25 + loss), f"accumulate: {float(acc)!r}"
    nody, _ = run_loss(dev, yh, kind, with_dy=False)
    assert bits_equal(nody, lv)                                        # the value does not depend on whether the gradient is asked for


# ---- 4. GRU ------------------------------------------------------------------------------------------------------------------------------------------------
def gru_forward(dev, o, T, B, dm):
    t = {k: o[k].float().contiguous().to(dev) for k in ("e", "h0", "w_ih", "w_hh", "b_ih", "b_hh")}
    out, gates = Flat(B * T * dm, dev), Flat(T * B * 4 * dm, dev)
    call("dcv_gru_forward", P(t["e"]), P(t["h0"]), P(t["w_ih"]), P(t["w_hh"]), P(t["b_ih"]), P(t["b_hh"]), P(out.v), P(gates.v), T, B, dm, S())
    return t, out, gates


@pytest.mark.parametrize("shape", E.GRU_SHAPES, ids=str)
def test_gru_layouts_exactly(dev, shape):
    T, B, dm = shape
    h0, e, want, wg = E.gru_layout_operands(T, B, dm)
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)
    o = dict(e=e, h0=h0, w_ih=z(3 * dm, dm), w_hh=z(3 * dm, dm), b_ih=z(3 * dm), b_hh=z(3 * dm))
    _, out, gates = gru_forward(dev, o, T, B, dm)
    got = out.get("gru out").view(B, T, dm)
    assert bits_equal(got, want.float()), "out (B, T, dm): " + X.first_mismatch(got.double() != want, got.double(), want, (B, T, dm), None)
    gg = gates.get("gru gates").view(T, B, 4, dm)
    assert bits_equal(gg, wg.float()), "gates [(t B + b) 4 dm + gate dm + u]: first mismatch at (t, b, gate, u) = " + str(tuple(int(v[0]) for v in (gg.double() != wg).nonzero(as_tuple=True)))


@pytest.mark.parametrize("shape", E.GRU_SHAPES, ids=str)
def test_gru_forward_and_backward_against_fp64_grucell(dev, shape):
    from dcvgan_amd import native as N
    T, B, dm = shape
    o = E.gru_operands(T, B, dm)
    r64, r32 = E.gru_unrolled(o, torch.float64), E.gru_unrolled(o, torch.float32)
    t, out, gates = gru_forward(dev, o, T, B, dm)
    got = {"out": out.get("gru out").view(B, T, dm)}
    _, want_gates = E.gru_plain(o)
    assert E.rel_l2(gates.get("gru gates").view(T, B, 4, dm), want_gates) < 1e-5      # (the layout is checked exactly above; this is the saved state the backward pass reads)
    dout = o["dout"].float().contiguous().to(dev)
    need = N.lib().dcv_gru_workspace_bytes(B, dm)
    ws = Flat(need // 4 + 1, dev)
    grads = {k: Flat(n, dev) for k, n in (("dw_ih", 3 * dm * dm), ("dw_hh", 3 * dm * dm), ("db_ih", 3 * dm), ("db_hh", 3 * dm))}
    args = [P(dout), P(t["e"]), P(t["h0"]), P(out.v), P(gates.v), P(t["w_ih"]), P(t["w_hh"])] + [P(grads[k].v) for k in ("dw_ih", "dw_hh", "db_ih", "db_hh")]
    L = N.lib()
    # a workspace one byte short: refused, nothing written
    assert L.dcv_gru_backward(*args, T, B, dm, P(ws.v), need - 1, S()) == N.DCV_EWORKSPACE
    sync()
    assert all(bool(torch.isnan(f.buf).all()) for f in grads.values()) and bool(torch.isnan(ws.buf).all())
    assert L.dcv_gru_forward(P(t["e"]), P(t["h0"]), P(t["w_ih"]), P(t["w_hh"]), P(t["b_ih"]), P(t["b_hh"]), P(out.v), P(gates.v), T, B, 33, S()) == N.DCV_EINVAL
    assert L.dcv_gru_backward(*args, T, B, 33, P(ws.v), 1 << 30, S()) == N.DCV_EINVAL
    call("dcv_gru_backward", *args, T, B, dm, P(ws.v), need, S())
    sync()
    assert ws.intact()
    for k, f in grads.items():
        got[k] = f.get(f"gru {k}").view(r64[k].shape)
    row = NOTES["gru"]["x".join(map(str, shape))] = {}
    fails = []
    for k in ("out", "dw_ih", "dw_hh", "db_ih", "db_hh"):
        e_cpu, e_hip = E.rel_l2(r32[k], r64[k]), E.rel_l2(got[k], r64[k])
        row[k] = {"e_cpu": e_cpu, "e_hip": e_hip}
        print(f"gru {shape} {k}: e_cpu {e_cpu:.3e} e_hip {e_hip:.3e}")
        if not E.gru_passes(e_hip, e_cpu):
            fails.append((k, e_hip, e_cpu))
    assert not fails, f"relative L2 error against the fp64 GRUCell beyond 5 max(e_cpu, 2e-7): {fails}"


# ---- 5. channel softmax / argmax -----------------------------------------------------------------------------------------------------------------------------
SM_PARAMS = [(s, i) for s in E.SM_SHAPES for i in range(5)]
SM_IDS = [f"{s}-{i}" for s, i in SM_PARAMS]


@pytest.mark.parametrize("shape,li", SM_PARAMS, ids=SM_IDS)
def test_softmax_channels(dev, shape, li):
    lin, lout = E.sm_layouts(shape[1])[li]
    xh, dyh = E.softmax_operands(shape)
    want = torch.softmax(xh, 1)
    x, y = g_in(shape, lin, dev, xh), Out(shape, lout, dev)
    call("dcv_softmax_channels_forward", P(x), D(x), P(y.view), D(y.view), S())
    r = y.check(f"softmax forward {lin} -> {lout}", want, E.softmax_forward_bound(want))
    print(f"softmax forward {shape} {lin} -> {lout}: worst error / bound {r:.3f}")
    got = y.view.detach().cpu()
    assert bool(torch.isfinite(got).all())
    yh = want.float().double()                                        # the backward pass's operand: fp32 values
    dy, yy, dx = g_in(shape, lin, dev, dyh), g_in(shape, lout, dev, yh), Out(shape, lin, dev)
    call("dcv_softmax_channels_backward", P(dy), D(dy), P(yy), D(yy), P(dx.view), D(dx.view), S())
    dyf = dyh.float().double()
    r = dx.check(f"softmax backward {lin}, {lout} -> {lin}", E.softmax_backward_ref(dyf, yh), E.softmax_backward_bound(dyf, yh))
    print(f"softmax backward {shape}: worst error / bound {r:.3f}")


@pytest.mark.parametrize("shape,li", SM_PARAMS, ids=SM_IDS)
def test_argmax_entries_take_the_first_maximum(dev, shape, li):
    lin, lout = E.sm_layouts(shape[1])[li]
    xh = E.argmax_operands(shape)
    x, y = g_in(shape, lin, dev, xh), Out(shape, lout, dev)
    call("dcv_segm_onehot", P(x), D(x), P(y.view), D(y.view), S())
    y.check(f"segm_onehot {lin} -> {lout}", E.onehot_ref(xh))
    pal = E.palette_of(shape[1])
    want = E.segm_rgb_ref(xh, pal)
    pd = torch.from_numpy(pal).to(dev)
    out = Flat(want.size, dev, torch.uint8)
    call("dcv_segm_to_rgb", P(x), D(x), P(pd), P(out.v), S())
    got = out.get("segm_to_rgb").numpy().reshape(want.shape)
    bad = got != want
    assert not bad.any(), f"segm_to_rgb {lin}: {int(bad.sum())} bytes differ, first at (n, k, d, h, w) = {tuple(int(v[0]) for v in np.nonzero(bad))}"


# ---- 6. flow visualisation -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["plain", "permuted"])
def test_flow_to_rgb_against_the_contract(dev, layout):
    """The header's contract restated in fp64 (tests/exactew.py::flow_rgb_ref).  Bytes whose fp64 value is decidable ("safe") must match, the others may differ
    by one.  cv2 is not available to the tests: parity with OpenCV's own cartToPolar / cvtColor stays unverified."""
    fh = E.flow_operands()
    want, safe = E.flow_rgb_ref(fh)
    B, _, T, H, W = E.FLOW_SHAPE
    f = g_in(E.FLOW_SHAPE, layout, dev, fh)
    out, mm = Flat(want.size, dev, torch.uint8), Flat(2 * B * T, dev)
    call("dcv_flow_to_rgb", P(f), D(f), E.FLOW_SCALE, P(out.v), P(mm.v), S())
    got = out.get("flow_to_rgb").numpy().reshape(want.shape).astype(np.int64)
    mm.get("flow_to_rgb min / max")
    diff = np.abs(got - want.astype(np.int64))
    bad = (diff > 0) & safe
    assert not bad.any(), f"{int(bad.sum())} decidable bytes differ, first at (b, k, t, h, w) = {tuple(int(v[0]) for v in np.nonzero(bad))}: got {got[bad][0]}, expected {want[bad][0]}"
    assert diff.max() <= 1, f"an undecidable byte is off by {diff.max()}"
    for bt in (E.FLOW_ZERO_FRAME, E.FLOW_CONST_FRAME):
        assert not got[bt // T, :, bt % T].any(), f"frame {bt} has no magnitude range and must be black"
    print(f"flow_to_rgb {layout}: {int((diff > 0).sum())} of {diff.size} bytes differ by one, all of them undecidable; safe share {safe.mean():.3f}")
