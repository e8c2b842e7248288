"""CPU: the host side of the exact elementwise / RNG / loss / GRU / softmax / flow checks (tests/exactew.py) against torch, numpy and the standard library —
a wrong restatement would make tests/test_ew_exact_gpu.py check the kernels against the wrong thing.  Also here: the path table covers every branch of the
fp32 dispatcher, each exactness claim holds for the chosen operands, the flow inputs leave at least 90 % of the bytes decidable, the argument checks that return
before any launch, and the recorded figures of tests/golden/ew_exact_notes.json are well-formed."""
import colorsys
import ctypes
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import exactbn as X
from tests import exactew as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOTES = os.path.join(ROOT, "tests", "golden", "ew_exact_notes.json")


# ---- 1. dispatcher -----------------------------------------------------------------------------------------------------------------------------------------
def test_case_table_reaches_every_path_of_the_dispatcher():
    seen = set()
    for c in E.EW_CASES:
        for combo in c.combos:
            for k in (1, 2, 3):
                path, d = E.ew_path(c.shape, E.operand_layouts(combo, k))
                assert path == c.path, (c.name, combo, k, path)
                seen.add(path)
    assert seen == E.EW_PATHS
    d = E.ew_path(E.ew_case("rows_1024").shape, ("plain",))[1]
    assert d.gpr == 256                                                  # one trip of ew_rows' loop
    d = E.ew_path(E.ew_case("rows_2048").shape, ("plain",))[1]
    assert d.gpr == 512                                                  # two trips
    d = E.ew_path(E.ew_case("stride_tail").shape, ("plain", "plain"))[1]
    assert d.groups == 2101250 > 8192 * 256 and d.ew_blocks == 8192 and d.groups % (8192 * 256) % 256 != 0      # the grid-stride loop, and a ragged last trip
    for name in ("degenerate_nc", "degenerate_w", "degenerate_d"):
        n, c, dd, h, w = X.five(E.ew_case(name).shape)
        assert 1 in (c * dd, dd, w) or h * w == 1                        # a divisor of 1 in a FastDiv


def test_lost_vec_layouts_remove_the_vector_path_one_operand_at_a_time():
    shape = E.ew_case("lost_vec").shape
    assert E.ew_path(shape, ("plain",) * 3)[0] == "ew<4>"
    for lay in ("misaligned", "nstride2"):
        for pos in range(3):
            lays = ["plain"] * 3
            lays[pos] = lay
            assert E.ew_path(shape, lays)[0] == "ew<1> inner!=1"


@pytest.mark.parametrize("name", [c.name for c in E.EW_CASES if not c.big])
def test_elementwise_expectations_are_exact_in_fp32(name):
    o = E.ew_operands(name, E.ew_case(name).shape)
    assert E.ew_exactness(o)
    x = o["x"].float().requires_grad_(True)
    y = F.leaky_relu(x, E.SLOPE)
    assert torch.equal(y.detach().double(), E.act_forward_ref(o["x"], "leaky"))
    y.backward(o["dy"].float())
    nz = o["x"] != 0                                                     # at 0 torch's derivative is the slope, as the kernel's y > 0 test gives
    assert torch.equal(x.grad.double(), E.act_backward_ref(o["dy"], E.act_forward_ref(o["x"], "leaky"), "leaky")) and bool(nz.any())
    t = o["yt"].float()
    assert torch.equal((o["dy"].float() * (1 - t * t)).double(), E.act_backward_ref(o["dy"], o["yt"], "tanh"))
    assert torch.equal((0.5 * o["x"].float() - 2 * o["z"].float()).double(), E.axpby_ref(o["x"], o["z"]))


def test_uint8_restatement_matches_torch_fp32():
    for rep in (1, 3):
        x = E.u8_operands("cpu", (2, 3, 2, 5, 7))
        t = torch.from_numpy(x)
        want = (((t.clamp(-1, 1) + 1) * 0.5) * 255).to(torch.int32).to(torch.uint8).repeat_interleave(rep, dim=1).numpy()
        got = E.to_u8_ref(x, rep)
        assert got.shape == (2, 3 * rep, 2, 5, 7) and np.array_equal(got, want)
        flat = got.reshape(2, 3, rep, -1)[0, 0, 0]
        # 1 - 2^-24: the fp32 sum (1 - 2^-24) + 1 is a tie and rounds to 2, so the byte is 255 as well (the fp32 operation order is what the bytes follow)
        assert flat[:10].tolist() == [255, 0, 127, 127, 255, 255, 0, 0, 255, 0]


# ---- 2. RNG ------------------------------------------------------------------------------------------------------------------------------------------------
def test_philox_words_follow_the_documented_counter_and_key_layout():
    seed, off = E.SEED_HI, E.OFFSET_HI
    w = E.philox_words(3, seed, off, q0=2 ** 32 + 1)
    for j in range(3):
        q = 2 ** 32 + 1 + j
        ctr = np.array([[q & E.M32, q >> 32, off & E.M32, off >> 32]], dtype=np.uint64)
        assert np.array_equal(w[j], E.philox4x32_10(ctr, (seed & E.M32, seed >> 32))[0])
    assert len({(seed >> 32), seed & E.M32, off >> 32, off & E.M32, 0}) == 5          # all four words set and different
    # every counter / key word matters: changing any one of them changes the words
    base = E.philox_words(1, seed, off)[0]
    for s2, o2 in ((seed ^ 1, off), (seed ^ (1 << 32), off), (seed, off ^ 1), (seed, off ^ (1 << 32))):
        assert not np.array_equal(base, E.philox_words(1, s2, o2)[0])
    z = E.philox_words(1, 0, 0)[0]
    assert [f"{int(v):08x}" for v in z] == ["6627e8d5", "e169c58d", "bc57ac4c", "9b00dbd8"]      # Salmon et al.'s known answer, through this wrapper


def test_normal_restatement_is_box_muller_of_the_fp32_uniforms():
    n = 131073
    z = E.normal_ref(n, E.SEED_HI, E.OFFSET_HI)
    assert z.shape == (n,) and abs(z.mean()) < 0.01 and abs(z.std() - 1) < 0.01
    u = E.u01(E.philox_words(4, 7, 9))
    zz = E.normal_ref(16, 7, 9).reshape(4, 4)
    assert np.allclose(zz[:, 0] ** 2 + zz[:, 1] ** 2, -2 * np.log(u[:, 0].astype(np.float64)), rtol=1e-12)
    assert np.allclose(zz[:, 2] ** 2 + zz[:, 3] ** 2, -2 * np.log(u[:, 2].astype(np.float64)), rtol=1e-12)
    assert np.allclose(np.arctan2(zz[:, 1], zz[:, 0]) % (2 * np.pi), (2 * np.pi * u[:, 1].astype(np.float64)) % (2 * np.pi), atol=1e-6)
    assert np.array_equal(E.normal_many_ref(5, 3, 7, 9)[2], E.normal_ref(5, 7, 11))
    assert np.array_equal(E.normal_ref(5, 7, 9), E.normal_ref(8, 7, 9)[:5])


def test_dropout_restatement():
    for p in E.DROPOUT_EXACT_P:
        keep = float(np.float32(1) / (np.float32(1) - np.float32(p)))
        assert keep == 2.0 ** round(np.log2(keep))                        # a power of two: the device's division cannot round differently
    m = E.dropout_ref(131073, 0.25, E.SEED_HI, E.OFFSET_HI)
    assert m.dtype == np.float32 and set(np.unique(m).tolist()) == {0.0, float(np.float32(1) / np.float32(0.75))}
    assert abs((m == 0).mean() - 0.25) < 0.01
    assert bool((E.dropout_ref(1025, 0.0, 1, 2) == 1).all())
    u = E.u01(E.philox_words(2, 5, 6)).reshape(-1)
    assert np.array_equal(E.dropout_ref(7, 0.5, 5, 6) != 0, u[:7] >= np.float32(0.5))


def test_cl_noise_restatement_orders_groups_fastest():
    shape = (2, 20, 1, 3, 5)
    z = E.cl_noise_ref(shape, 3, 4)
    G, PIX = 3, 15
    for (n, c, pix) in ((0, 0, 0), (0, 9, 0), (0, 3, 1), (1, 19, 14)):
        i, e = (n * PIX + pix) * G + c // 8, c % 8
        want = E.normals_of_words(E.philox_words(1, 3, 4, q0=2 * i + e // 4))[0, e % 4]
        assert z[n, c, 0, pix // 5, pix % 5] == want
    assert abs(E.half_ulp(np.array([1.0]), torch.bfloat16)[0] - 2.0 ** -8) == 0 and abs(E.half_ulp(np.array([3.0]), torch.float16)[0] - 2.0 ** -10) == 0


# ---- 3. GAN losses -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1, 2, 3, 4])
def test_gan_loss_restatement_matches_torch_fp64(kind):
    for n in E.LOSS_N:
        y = torch.from_numpy(E.loss_logits(n, kind)).requires_grad_(True)
        want = {0: lambda v: F.binary_cross_entropy_with_logits(v, torch.ones_like(v)), 1: lambda v: F.binary_cross_entropy_with_logits(v, torch.zeros_like(v)),
                2: lambda v: F.relu(1 - v).mean(), 3: lambda v: F.relu(1 + v).mean(), 4: lambda v: F.softplus(-v).mean()}[kind](y)
        want.backward()
        f, g = E.gan_loss_ref(y.detach().numpy(), kind)
        assert abs(f.sum() / n - float(want.detach())) <= 1e-14 * max(1.0, abs(float(want.detach())))
        assert np.allclose(g / n, y.grad.numpy(), rtol=1e-12, atol=1e-15)      # torch forms sigmoid(v) - 1: it cancels where ours does not
        v = y.detach().numpy()
        assert bool(np.array_equal(v.astype(np.float32).astype(np.float64), v))
        if kind in E.HINGE_KINDS:
            assert (n == 1 or (1.0 in v and -1.0 in v)) and bool(np.all(v * 2 == np.round(v * 2))) and np.abs(v).max() <= 4
            loss, dy = E.hinge_expected(v, kind)
            assert loss.dtype == np.float32 and dy.dtype == np.float32
            edge = v == (1.0 if kind == 2 else -1.0)
            assert bool((dy[edge] == 0).all())                           # g = 0 at the boundary, as torch's relu' gives
            assert bool((y.grad.numpy()[edge] == 0).all())
        else:
            if n > 6:
                assert all(p in v for p in (20.0, -20.0, 88.0, -88.0, 100.0, -100.0))
            loss, bl, dy, bdy = E.softplus_bounds(v, kind)
            assert np.isfinite(loss) and np.isfinite(dy).all() and bl < 2e-6 * max(1.0, loss) and bool((bdy <= 14 * E.U * np.abs(dy) * 1.01 + E.TINY).all())


# ---- 4. GRU ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", E.GRU_SHAPES, ids=str)
def test_gru_restatements(shape):
    T, B, dm = shape
    o = E.gru_operands(T, B, dm)
    r64 = E.gru_unrolled(o, torch.float64)
    out, gates = E.gru_plain(o)
    assert out.shape == (B, T, dm) and gates.shape == (T, B, 4, dm)
    assert E.rel_l2(out, r64["out"]) < 1e-14
    r32 = E.gru_unrolled(o, torch.float32)
    for k in ("out", "dw_ih", "dw_hh", "db_ih", "db_hh"):
        assert E.rel_l2(r32[k], r64[k]) < 1e-5, k
    # the layout scheme: torch's fp32 GRUCell with zero parameters halves the state exactly
    h0, e, want, g = E.gru_layout_operands(T, B, dm)
    z = dict(e=e, h0=h0, dout=torch.zeros(B, T, dm, dtype=torch.float64), w_ih=torch.zeros(3 * dm, dm), w_hh=torch.zeros(3 * dm, dm), b_ih=torch.zeros(3 * dm), b_hh=torch.zeros(3 * dm))
    assert torch.equal(E.gru_unrolled(z, torch.float32)["out"].double(), want)
    o2, g2 = E.gru_plain({k: v.double() for k, v in z.items()})
    assert torch.equal(o2, want) and torch.equal(g2, g)
    assert len(set(h0.reshape(-1).tolist())) == B * dm
    assert not E.gru_passes(1e-5, 1e-7) and E.gru_passes(9e-7, 1e-9) and E.gru_passes(4e-6, 1e-6)


# ---- 5. softmax / argmax -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", E.SM_SHAPES, ids=str)
def test_softmax_and_argmax_restatements(shape):
    x, dy = E.softmax_operands(shape)
    y = torch.softmax(x, 1)
    assert bool(torch.isfinite(y).all()) and float((y.sum(1) - 1).abs().max()) < 1e-14
    xs = x.clone().requires_grad_(True)
    torch.softmax(xs, 1).backward(dy)
    assert torch.allclose(E.softmax_backward_ref(dy, y), xs.grad, rtol=1e-10, atol=1e-300)
    assert float(E.softmax_forward_bound(y).max()) <= (8 + shape[1]) * E.U + E.TINY
    a = E.argmax_operands(shape)
    idx = E.argmax_first(a)
    assert torch.equal(idx, torch.argmax(a, 1))
    C = shape[1]
    assert int(idx[0, 0, 0, 0]) == 0 and int(idx[0, 0, 0, 1]) == 0 and int(idx[0, 0, 0, 2]) == max(C - 2, 0)
    ties = (a == a.max(1, keepdim=True).values).sum(1) > 1
    assert C == 1 or int(ties.sum()) > 3
    oh = E.onehot_ref(a)
    assert bool(((oh == 1).sum(1) == 1).all()) and bool(((oh == 1) | (oh == -1)).all())
    pal = E.palette_of(C)
    rgb = E.segm_rgb_ref(a, pal)
    assert rgb.shape == (shape[0], 3) + tuple(shape[2:]) and rgb.dtype == np.uint8
    assert rgb[0, :, 0, 0, 2].tolist() == pal[max(C - 2, 0)].tolist()
    assert len({tuple(r) for r in pal.tolist()}) == C


# ---- 6. flow -----------------------------------------------------------------------------------------------------------------------------------------------
def test_flow_restatement_and_safe_share():
    f = E.flow_operands()
    B, _, T, H, W = E.FLOW_SHAPE
    assert B * T == 6 and (H, W) == (5, 13) and bool(X.is_f32(f).all())
    rgb, safe = E.flow_rgb_ref(f)
    assert rgb.shape == (B, 3, T, H, W) and safe.shape == rgb.shape
    assert safe.mean() >= 0.9, safe.mean()                                # the issue's condition
    fr = lambda bt: rgb[bt // T, :, bt % T]
    assert not fr(E.FLOW_ZERO_FRAME).any() and not fr(E.FLOW_CONST_FRAME).any()      # black: no magnitude range
    assert fr(0).any() and fr(E.FLOW_CLIP_FRAME).any()
    # hue: every direction at least half a bucket from an edge
    x, y = np.clip(f[:, 0].numpy(), -1, 1), np.clip(f[:, 1].numpy(), -1, 1)
    live = (x != 0) | (y != 0)
    live[E.FLOW_CONST_FRAME // T, E.FLOW_CONST_FRAME % T] = False
    half = (np.degrees(np.arctan2(y, x)) % 360) / 2.0
    assert np.abs(half[live] - np.floor(half[live]) - 0.5).max() < 1e-4
    # the sector formula against colorsys, per pixel
    mg = np.sqrt(x * x + y * y) * E.FLOW_SCALE
    for b in range(B):
        for t in range(T):
            lo, hi = mg[b, t].min(), mg[b, t].max()
            for h in range(H):
                for w in range(W):
                    V = int(np.floor((mg[b, t, h, w] - lo) * (255.0 / (hi - lo)))) if hi > lo else 0
                    hh = int(np.floor(half[b, t, h, w]))
                    want = [int(c + 0.5) for c in colorsys.hsv_to_rgb(hh / 180.0, 1.0, float(V))]
                    got = rgb[b, :, t, h, w].tolist()
                    assert all(abs(p - q) <= (0 if s else 1) for p, q, s in zip(got, want, safe[b, :, t, h, w])), (b, t, h, w, got, want)


# ---- argument checks that return before any launch ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from dcvgan_amd import native
    if not os.path.exists(native.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return native.lib()


def test_null_dims_and_gru_sizes_are_refused_on_the_host(lib):
    from dcvgan_amd import native
    from dcvgan_amd.native import Dims5
    fake = ctypes.create_string_buffer(64)      # never dereferenced
    a = ctypes.addressof(fake)
    d = Dims5(2, 3, 2, 8, 8, 384, 128, 64, 8, 1)
    r = ctypes.byref(d)
    n0 = lib.dcv_launch_count()
    EINVAL = native.DCV_EINVAL
    assert lib.dcv_act_forward(a, None, a, r, 1, 0.25, None) == EINVAL and lib.dcv_act_forward(a, r, a, None, 1, 0.25, None) == EINVAL
    for dims in ((None, r, r), (r, None, r), (r, r, None)):
        assert lib.dcv_act_backward(a, dims[0], a, dims[1], a, dims[2], 1, 0.25, None) == EINVAL
        assert b"act_backward" in lib.dcv_last_error()
    assert lib.dcv_act_backward(None, r, a, r, a, r, 1, 0.25, None) == EINVAL
    for dims in ((None, r), (r, None)):
        assert lib.dcv_noise_add(a, dims[0], a, dims[1], 0.5, 1, 2, None) == EINVAL
        assert b"noise_add" in lib.dcv_last_error()
    assert lib.dcv_axpby(a, r, 0.5, a, None, -2.0, a, r, None) == EINVAL          # z without its dims
    assert lib.dcv_axpby(a, None, 0.5, a, r, -2.0, a, r, None) == EINVAL and lib.dcv_axpby(a, r, 0.5, a, r, -2.0, a, None, None) == EINVAL
    assert lib.dcv_axpby(a, None, 0.5, None, None, 0.0, a, r, None) == EINVAL
    # GRU: dm = 33 from both entries; T, B, dm >= 1; a workspace one byte short
    fwd = lambda T, B, dm: lib.dcv_gru_forward(a, a, a, a, a, a, a, a, T, B, dm, None)
    bwd = lambda T, B, dm, ws: lib.dcv_gru_backward(a, a, a, a, a, a, a, a, a, a, a, T, B, dm, a, ws, None)
    big = 1 << 30
    assert fwd(4, 2, 33) == EINVAL and bwd(4, 2, 33, big) == EINVAL
    for bad in ((0, 2, 8), (4, 0, 8), (4, 2, 0), (-1, 2, 8)):
        assert fwd(*bad) == EINVAL and bwd(*bad, big) == EINVAL, bad
    need = lib.dcv_gru_workspace_bytes(2, 32)
    assert need >= 2 * (6 * 32 * 32 + 6 * 32) * 4
    assert bwd(4, 2, 32, need - 1) == native.DCV_EWORKSPACE
    assert lib.dcv_gru_backward(a, a, a, a, a, a, a, a, a, a, a, 4, 2, 32, None, need, None) == native.DCV_EWORKSPACE
    assert lib.dcv_launch_count() == n0


# ---- the recorded figures ----------------------------------------------------------------------------------------------------------------------------------
def test_recorded_figures_are_well_formed():
    notes = json.load(open(NOTES))
    for key in ("normal_fill_max_err", "cl_noise_max_err"):
        v = notes[key]
        assert v is None or 0 <= v <= E.NORMAL_CAP * 1.01, (key, v)       # None: not measured (the file says so under "measured_on")
    assert isinstance(notes["measured_on"], str)
    for shape in E.GRU_SHAPES:
        row = notes["gru"]["x".join(map(str, shape))]
        for k in ("out", "dw_ih", "dw_hh", "db_ih", "db_hh"):
            e_cpu, e_hip = row[k]["e_cpu"], row[k]["e_hip"]
            assert e_cpu >= 0 and (e_hip is None or e_hip >= 0)
