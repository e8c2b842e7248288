"""CPU: the LeCam regulariser's binding, and its NORMATIVE restatement in numpy.

`sums_ref` and `apply_ref` say what dcv_lecam_sums and dcv_lecam_apply compute, bit for bit, over a `state` of 8-word lists (include/dcvgan_hip.h: DCV_LECAM_*);
tests/test_lecam_gpu.py holds the kernels to them with exact equality.  Here the restatement itself is checked: its gradient against float64 autograd of the
published formula, the anchors' recursion against its closed form, the inactive and the non-finite rule."""
import ctypes
import inspect
import os
import re
import struct

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dcv_lecam_sums", "dcv_lecam_apply")
F32, F64 = np.float32, np.float64
ANCHOR_REAL, ANCHOR_FAKE, UPDATES, ACTIVE, STATE_WORDS = 0, 1, 2, 3, 8
LANES = 256


def f32_bits(v) -> int:
    return struct.unpack("<i", struct.pack("<f", float(v)))[0]


def bits_f32(b) -> np.float32:
    return np.array([int(b) & 0xFFFFFFFF], dtype=np.uint32).view(F32)[0]


def zero_state(n_dis):
    return [[0] * STATE_WORDS for _ in range(n_dis)]


# ---- the specification ------------------------------------------------------------------------------------------------------------------------------------
def lane_sum(v) -> np.float64:
    """THE sum order of both kernels.  v: float64 values.  Lane l of 256 adds elements l, l + 256, ... in increasing index into a double that starts at +0.0; then
    for s = 128, 64, .., 1 every lane l < s does p[l] += p[l + s]; the result is p[0]."""
    v = np.asarray(v, dtype=F64).reshape(-1)
    rows = -(-v.size // LANES)
    padded = np.zeros(rows * LANES, dtype=F64)
    padded[:v.size] = v
    grid, live = padded.reshape(rows, LANES), np.arange(rows * LANES).reshape(rows, LANES) < v.size
    p = np.zeros(LANES, dtype=F64)
    with np.errstate(all="ignore"):
        for r in range(rows):      # a lane without an element r adds nothing (not even +0.0 to a -0.0: there is none, p starts at +0.0)
            p = np.where(live[r], p + grid[r], p)
        s = LANES // 2
        while s >= 1:
            p[:s] = p[:s] + p[s:2 * s]
            s //= 2
    return p[0]


def sums_ref(y_reals, y_fakes):
    """-> (n_dis, 4) float64: {sum y_real, n_real, sum y_fake, n_fake} per discriminator, what dcv_lecam_sums writes."""
    return np.array([[lane_sum(np.asarray(yr, dtype=F32).astype(F64)), F64(np.asarray(yr).size), lane_sum(np.asarray(yf, dtype=F32).astype(F64)), F64(np.asarray(yf).size)]
                     for yr, yf in zip(y_reals, y_fakes)], dtype=F64).reshape(-1, 4)


def _side(y, anchor, sign, one_sided):
    """d = y - anchor (sign +1, the real side) or anchor - y (sign -1, the fake side): one fp32 subtraction; one-sided: d < 0 -> 0 (a NaN stays a NaN)."""
    y = np.asarray(y, dtype=F32).reshape(-1)
    with np.errstate(all="ignore"):
        d = (y - F32(anchor)) if sign > 0 else (F32(anchor) - y)
        if one_sided:
            d = np.where(d < 0, F32(0), d)
    return d.astype(F32)


def apply_ref(y_reals, y_fakes, sums, state, decay, start, weight, one_sided, losses, dy_reals, dy_fakes):
    """What dcv_lecam_apply does.  sums: (n_dis, 4) float64 (sums_ref's, or all-reduced); state: n_dis lists of 8 words; losses: n_dis fp32 scalars; dy_*: fp32
    arrays shaped like the logits.  -> (state', losses', dy_reals', dy_fakes', reg) as new objects; the inputs are not modified."""
    weight, decay = F64(weight), F64(decay)
    out_state, out_loss, out_dr, out_df, reg = [], [], [], [], []
    with np.errstate(all="ignore"):
        for k, (yr, yf) in enumerate(zip(y_reals, y_fakes)):
            st = list(state[k])
            aR, aF, U = bits_f32(st[ANCHOR_REAL]), bits_f32(st[ANCHOR_FAKE]), int(st[UPDATES])
            # 1. the switch
            active = U >= max(int(start), 1)
            st[ACTIVE] = 1 if active else 0
            # 2. the regulariser, with the OLD anchors
            n_r, n_f = np.asarray(yr).size, np.asarray(yf).size
            d, e = _side(yr, aF, +1, one_sided), _side(yf, aR, -1, one_sided)
            S_d, S_e = lane_sum(d.astype(F64) * d.astype(F64)), lane_sum(e.astype(F64) * e.astype(F64))
            R = S_d / F64(n_r) + S_e / F64(n_f)
            r = F32(weight * R)
            loss, dr, df = F32(losses[k]), np.array(dy_reals[k], dtype=F32, copy=True), np.array(dy_fakes[k], dtype=F32, copy=True)
            if active:
                c_r, c_f = F32(F64(2.0) * weight / F64(n_r)), F32(F64(2.0) * weight / F64(n_f))
                loss = F32(loss + r)
                dr = (dr.reshape(-1) + (c_r * d).astype(F32)).astype(F32).reshape(dr.shape)      # product and sum rounded on their own
                df = (df.reshape(-1) - (c_f * e).astype(F32)).astype(F32).reshape(df.shape)
            reg.append(r if active else F32(0))
            # 3. the anchors
            m_r, m_f = F64(sums[k][0]) / F64(sums[k][1]), F64(sums[k][2]) / F64(sums[k][3])
            if np.isfinite(m_r) and np.isfinite(m_f):
                if U == 0:
                    aR, aF = F32(m_r), F32(m_f)
                else:
                    w = F64(1.0) - decay
                    aR, aF = F32(F64(aR) * decay + m_r * w), F32(F64(aF) * decay + m_f * w)
                st[ANCHOR_REAL], st[ANCHOR_FAKE], st[UPDATES] = f32_bits(aR), f32_bits(aF), U + 1
            out_state.append(st); out_loss.append(loss); out_dr.append(dr); out_df.append(df)
    return out_state, out_loss, out_dr, out_df, np.array(reg, dtype=F32)


# ---- the binding --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from dcvgan_amd import native
    if not os.path.exists(native.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return native.lib()


def test_new_names_are_bound_declared_and_exported(lib):
    from dcvgan_amd import lecam, native
    header = open(os.path.join(ROOT, "include", "dcvgan_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    raw = ctypes.CDLL(native.LIB_PATH)
    for n in NEW:
        assert n in native.EXPORTS, n
        assert re.search(r"\b%s\s*\(" % n, code), f"{n} is not declared in dcvgan_hip.h"
        assert hasattr(raw, n), f"{n} is not exported by the library"
    assert lib.dcv_version() == native.ABI_VERSION == 4
    for name, value in (("ANCHOR_REAL", 0), ("ANCHOR_FAKE", 1), ("UPDATES", 2), ("ACTIVE", 3), ("STATE_WORDS", 8)):
        assert re.search(r"#define\s+DCV_LECAM_%s\s+%d\b" % (name, value), header), name
        assert getattr(lecam, name) == value
    assert re.search(r"for f in [^;]*\blecam\b", open(os.path.join(ROOT, "dcvgan_amd", "csrc", "build.sh")).read()), "csrc/lecam.hip is not in build.sh's list"


def test_arguments_and_defaults():
    from dcvgan_amd import lecam, trainer
    sig = inspect.signature(trainer.StepRunner.__init__)
    assert sig.parameters["lecam"].default is None and callable(trainer.build_lecam)
    p = inspect.signature(lecam.LeCam.__init__).parameters
    assert p["weight"].default is inspect.Parameter.empty and p["n_dis"].default == 3
    assert (p["decay"].default, p["start"].default, p["one_sided"].default) == (0.99, 1000, True)
    with pytest.raises(TypeError):
        lecam.LeCam(3, device="cpu")
    for bad in (dict(weight=-1.0), dict(weight=float("nan")), dict(weight=1.0, decay=1.5), dict(weight=1.0, start=-1), dict(weight=1.0, n_dis=9)):
        with pytest.raises(ValueError):
            lecam.LeCam(device="cpu", **bad)


def test_refusals_need_no_gpu(lib):
    """The argument checks run on the host before any launch."""
    import torch
    from dcvgan_amd import lecam, loss, native
    fake = ctypes.create_string_buffer(64)      # never dereferenced
    a = ctypes.addressof(fake)
    tab = lambda n, v=a: (ctypes.c_void_p * max(n, 1))(*([v] * max(n, 1)))
    cnt = lambda n, v: (ctypes.c_int64 * max(n, 1))(*([v] * max(n, 1)))
    n0 = lib.dcv_launch_count()

    def apply(n_dis, n_real=4, n_fake=4, decay=0.99, weight=0.1, tables=None):
        t = tables if tables is not None else tab(n_dis)
        return lib.dcv_lecam_apply(n_dis, t, t, cnt(n_dis, n_real), cnt(n_dis, n_fake), a, a, decay, 0, weight, 1, t, t, t, a, None)

    assert apply(0) == native.DCV_EINVAL and b"n_dis" in lib.dcv_last_error()
    assert apply(9) == native.DCV_EINVAL
    assert apply(3, n_real=0) == native.DCV_EINVAL and b"2^24" in lib.dcv_last_error()
    assert apply(3, n_fake=0) == native.DCV_EINVAL
    assert apply(1, n_real=(1 << 24) + 1) == native.DCV_EINVAL
    assert apply(3, decay=1.5) == native.DCV_EINVAL and apply(3, weight=-1.0) == native.DCV_EINVAL and apply(3, weight=float("nan")) == native.DCV_EINVAL
    assert apply(2, tables=tab(2, None)) == native.DCV_EINVAL
    assert lib.dcv_lecam_sums(0, tab(1), tab(1), cnt(1, 4), cnt(1, 4), a, None) == native.DCV_EINVAL
    assert lib.dcv_lecam_sums(2, tab(2), tab(2), cnt(2, 0), cnt(2, 4), a, None) == native.DCV_EINVAL
    assert lib.dcv_lecam_sums(2, tab(2), tab(2), cnt(2, 4), cnt(2, 4), None, None) == native.DCV_EINVAL
    assert lib.dcv_launch_count() == n0
    # Python: anything that is not an fp32 device tensor is refused, and so is a loss whose kinds are unknown
    lc = lecam.LeCam(3, weight=0.1, device="cpu")
    y = [torch.zeros(2, 1) for _ in range(3)]
    with pytest.raises(native.NativeError):
        lc.compute_dis_losses(loss.HingeLoss(), y, y)
    with pytest.raises(native.NativeError):
        lc.compute_dis_losses(loss.HingeLoss(), y[:2], y[:2])
    with pytest.raises(native.NativeError):
        lc.compute_dis_losses(object(), y, y)
    assert lecam.dis_kinds(loss.AdversarialLoss()) == (0, 1) and lecam.dis_kinds(loss.HingeLoss()) == (2, 3)
    sd = lc.state_dict()
    assert sd["state"] == zero_state(3)
    sd["state"][1][:3] = [f32_bits(0.5), f32_bits(-0.25), 7]
    lc.load_state_dict(sd)
    assert lc.state_words() == sd["state"] and lc.anchor_values()[1] == (0.5, -0.25) and tuple(lc.anchors().shape) == (3, 8)
    with pytest.raises(ValueError):
        lc.load_state_dict(dict(sd, state=sd["state"][:2]))
    assert lib.dcv_launch_count() == n0


# ---- the restatement itself -----------------------------------------------------------------------------------------------------------------------------------
def _logits(seed, sizes, scale=1.5):
    g = np.random.default_rng(seed)
    return [(g.standard_normal(n) * scale).astype(F32) for n in sizes]


def test_lane_sum_order():
    """Integers: any order gives the same sum; and one hand-made case where the order shows."""
    v = np.arange(1, 1001, dtype=F64)
    assert lane_sum(v) == 500500.0 and lane_sum([]) == 0.0 and lane_sum([-0.0]) == 0.0 and np.signbit(lane_sum([-0.0])) == False      # noqa: E712
    # lane 0 holds 2^53 + 2 (elements 0 and 256) before the tree; lane 128's 1 joins at s = 128: 2^53 + 3 ties to even, 2^53 + 4; lane 1's 1 at s = 1 changes
    # nothing.  Left to right the two ones are lost one by one and the sum is 2^53 + 2.
    w = np.zeros(257, dtype=F64)
    w[0], w[128], w[1], w[256] = 2.0 ** 53, 1.0, 1.0, 2.0
    seq = F64(0)
    for x in w:
        seq = seq + x
    assert lane_sum(w) == 2.0 ** 53 + 4.0 and seq == 2.0 ** 53 + 2.0
    y = _logits(1, [1123])[0].astype(F64)
    assert abs(lane_sum(y) - float(np.sum(y.astype(np.longdouble)))) <= 1123 * 2.0 ** -53 * float(np.sum(np.abs(y)))


@pytest.mark.parametrize("one_sided", [True, False])
def test_gradient_is_the_published_formula(one_sided):
    """apply_ref's value and gradient (from zero dy) against float64 autograd of weight * (mean(relu(y_r - aF)^2) + mean(relu(aR - y_f)^2)) (two-sided: without the
    relu).  Tolerance 4 x 2^-23 relative: the definition rounds to fp32 three times per element (the subtraction, c, their product); the reference is float64."""
    import torch
    sizes_r, sizes_f = [1, 255, 1123], [1, 257, 4099]
    yr, yf = _logits(2, sizes_r), _logits(3, sizes_f)
    aR, aF = [0.75, -0.125, 0.3], [-0.5, 0.0625, -0.2]
    state = [[f32_bits(a), f32_bits(b), 5, 0, 0, 0, 0, 0] for a, b in zip(aR, aF)]
    weight = 0.3
    z = lambda ys: [np.zeros_like(y) for y in ys]
    st, loss, dr, df, reg = apply_ref(yr, yf, sums_ref(yr, yf), state, 0.99, 0, weight, one_sided, [F32(0)] * 3, z(yr), z(yf))
    tol = 4 * 2.0 ** -23
    for k in range(3):
        tr, tf = torch.tensor(yr[k].astype(F64), requires_grad=True), torch.tensor(yf[k].astype(F64), requires_grad=True)
        a_r, a_f = float(F32(aR[k])), float(F32(aF[k]))
        d, e = tr - a_f, a_r - tf
        if one_sided:
            d, e = torch.relu(d), torch.relu(e)
        val = weight * ((d ** 2).mean() + (e ** 2).mean())
        val.backward()
        gr, gf = tr.grad.numpy(), tf.grad.numpy()
        assert st[k][ACTIVE] == 1 and st[k][UPDATES] == 6
        # the value: every d carries one fp32 rounding (2^-24), its square 2^-23, and so does the sum of squares; one more rounding to fp32 -> within 2^-22
        assert abs(float(reg[k]) - float(val.detach())) <= 2.0 ** -22 * abs(float(val.detach())) and loss[k] == reg[k]
        assert np.all(np.abs(dr[k].astype(F64) - gr) <= tol * np.abs(gr)), k
        assert np.all(np.abs(df[k].astype(F64) - gf) <= tol * np.abs(gf)), k
        assert one_sided or (np.count_nonzero(dr[k]) == dr[k].size and np.count_nonzero(df[k]) == df[k].size)
        if one_sided and sizes_r[k] > 1:
            assert 0 < np.count_nonzero(dr[k]) < dr[k].size and 0 < np.count_nonzero(df[k]) < df[k].size      # both branches of the relu ran


def test_anchor_recursion_against_its_closed_form():
    """Three updates from a zeroed state: a1 = m1; a2 = decay a1 + (1 - decay) m2; a3 = decay^2 m1 + decay (1 - decay) m2 + (1 - decay) m3, each held to one fp32
    rounding per update (2^-24 relative each, accumulated)."""
    decay = 0.9
    batches = [(_logits(10 + i, [300])[0] + F32(i), _logits(20 + i, [77])[0] - F32(i)) for i in range(3)]
    state, means = zero_state(1), []
    for i, (yr, yf) in enumerate(batches):
        s = sums_ref([yr], [yf])
        means.append((s[0][0] / s[0][1], s[0][2] / s[0][3]))
        state, _, _, _, reg = apply_ref([yr], [yf], s, state, decay, 1000, 0.1, True, [F32(0)], [np.zeros_like(yr)], [np.zeros_like(yf)])
        assert state[0][UPDATES] == i + 1 and state[0][ACTIVE] == 0 and reg[0] == 0
        if i == 0:
            assert state[0][ANCHOR_REAL] == f32_bits(F32(means[0][0])) and state[0][ANCHOR_FAKE] == f32_bits(F32(means[0][1]))
    for side, word in ((0, ANCHOR_REAL), (1, ANCHOR_FAKE)):
        m = [mm[side] for mm in means]
        closed = decay ** 2 * m[0] + decay * (1 - decay) * m[1] + (1 - decay) * m[2]
        bound = 3 * 2.0 ** -24 * (abs(m[0]) + abs(m[1]) + abs(m[2]))
        assert abs(float(bits_f32(state[0][word])) - closed) <= bound, (side, float(bits_f32(state[0][word])), closed)
    assert all(w == 0 for w in state[0][4:])


def test_inactive_call_returns_its_inputs_unchanged():
    yr, yf = _logits(4, [32, 256]), _logits(5, [128, 256])
    g = np.random.default_rng(6)
    dr, df = [g.standard_normal(y.shape).astype(F32) for y in yr], [g.standard_normal(y.shape).astype(F32) for y in yf]
    loss = [F32(0.7), F32(-1.25)]
    state = [[f32_bits(0.5), f32_bits(-0.5), 1, 1, 0, 0, 0, 0], [0] * 8]      # U = 1 < start = 2; U = 0 is never active
    st, l2, dr2, df2, reg = apply_ref(yr, yf, sums_ref(yr, yf), state, 0.99, 2, 0.1, True, loss, dr, df)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(dr + df, dr2 + df2)) and [f32_bits(v) for v in l2] == [f32_bits(v) for v in loss]
    assert not reg.any() and [s[ACTIVE] for s in st] == [0, 0] and [s[UPDATES] for s in st] == [2, 1]
    assert st[0][:2] != state[0][:2] and st[1][:2] != state[1][:2]      # the anchors moved all the same
    # start = 0 behaves as start = 1: the first call only initialises the anchors, the second is active
    st0, _, _, _, reg0 = apply_ref(yr, yf, sums_ref(yr, yf), [[0] * 8, [0] * 8], 0.99, 0, 0.1, True, loss, dr, df)
    assert not reg0.any() and [s[ACTIVE] for s in st0] == [0, 0]
    st1, l3, _, _, reg1 = apply_ref(yr, yf, sums_ref(yr, yf), st0, 0.99, 0, 0.1, True, loss, dr, df)
    assert reg1.all() and [s[ACTIVE] for s in st1] == [1, 1] and all(F32(a + b) == c for a, b, c in zip(loss, reg1, l3))


def test_non_finite_mean_leaves_the_state_unchanged():
    yr, yf = _logits(7, [64, 64]), _logits(8, [64, 64])
    state = [[f32_bits(0.5), f32_bits(-0.5), 3, 0, 0, 0, 0, 0], [f32_bits(0.25), f32_bits(-0.25), 3, 0, 0, 0, 0, 0]]
    z = lambda ys: [np.zeros_like(y) for y in ys]
    for bad in (np.nan, np.inf, -np.inf):
        y = [yr[0].copy(), yr[1]]
        y[0][17] = bad
        st, _, _, _, _ = apply_ref(y, yf, sums_ref(y, yf), state, 0.99, 1000, 0.1, True, [F32(0)] * 2, z(y), z(yf))
        assert st[0] == state[0], bad                       # anchors, UPDATES (and ACTIVE, 0 as before)
        assert st[1][UPDATES] == 4 and st[1][:2] != state[1][:2]
    # all-reduced sums that are not finite, or a zero count, do the same
    s = sums_ref(yr, yf)
    s[0][3] = 0.0
    st, _, _, _, _ = apply_ref(yr, yf, s, state, 0.99, 1000, 0.1, True, [F32(0)] * 2, z(yr), z(yf))
    assert st[0] == state[0] and st[1][UPDATES] == 4


def test_exact_logits_sum_exactly():
    """Multiples of 2^-8 below 8 in magnitude: every partial sum of up to 2^24 of them is an integer multiple of 2^-8 below 2^27 — exact in a double, whatever the
    order.  (The data-parallel test relies on it: a sum of two ranks' sums is then the sum over the concatenated logits, bit for bit.)"""
    g = np.random.default_rng(9)
    y = (g.integers(-2047, 2048, size=5000).astype(F64) / 256.0).astype(F32)
    s = sums_ref([y[:1234]], [y[1234:]])
    assert s[0][0] == float(np.sum(y[:1234].astype(F64))) and s[0][2] == float(np.sum(y[1234:].astype(F64)))
    a, b = sums_ref([y[:600]], [y[1234:3000]]), sums_ref([y[600:1234]], [y[3000:]])
    assert np.array_equal(a + b, s)
