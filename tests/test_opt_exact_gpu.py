"""GPU: the Adam, gradient-guard, guarded-Adam and EMA kernels of csrc/elementwise.hip against the host mirrors of tests/exactopt.py, BIT FOR BIT, through the C ABI.

Every tensor of a case is a view inside one buffer of NaN words (tests/exactopt.py, Arena): a band before, between and after the tensors.  A comparison is made on the
32-bit words of the WHOLE buffer, bands included, so a write outside a tensor is a mismatch like any other.  Values depend on the position (no two elements of a
case are equal), so a mis-addressed element cannot match by chance.  A mismatch is reported by tensor, element, table, slot, block, thread and trip, and for Adam
by which of m, v, p differed first: m names the lerp, v the addcmul, p the sqrt / divide tail.  Run with -s for the tallies DESIGN §7d and
tests/golden/opt_exact_notes.json quote."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from tests import exactopt as E

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F32, F64, U32, U64, I32 = np.float32, np.float64, np.uint32, np.uint64, np.int32
REF_HP = (2e-4, 0.5, 0.999, 1e-8, 1e-5)                    # lr, beta1, beta2, eps, weight decay: the reference's; w1 = 0.5 takes lerp's second branch
HPS = {"reference": REF_HP, "first_branch": (1e-3, 0.9, 0.999, 1e-8, 0.0), "beta1_0": (2e-4, 0.0, 0.999, 1e-8, 1e-5)}
GSCALES = (1.0, 0.125, 1.0 / 3.0)
TALLY = {}


def _tally(group, cases, words):
    t = TALLY.setdefault(group, {"cases": 0, "words": 0, "mismatches": 0})
    t["cases"] += cases
    t["words"] += int(words)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\n[opt-exact tallies] " + json.dumps(TALLY, sort_keys=True))


def _lib():
    from dcvgan_amd import native
    return native.lib()


def _dev(buf):
    t = torch.from_numpy(np.ascontiguousarray(buf)).to(DEV)
    assert t.data_ptr() % 16 == 0
    return t


def _host(t):
    return t.cpu().numpy()


def _ptrs(t, arena, null_empty=False):
    from dcvgan_amd.native import c_array
    return c_array([0 if (null_empty and n == 0) else t.data_ptr() + 4 * s for s, n in zip(arena.start, arena.sizes)])


def _numel(arena):
    from dcvgan_amd.native import c_array
    return c_array(arena.sizes, C.c_int64)


def _same(arena, got_t, want_buf, what, order=E.STRIDED):
    bad = E.first_mismatch(arena, _host(got_t), want_buf, order)
    assert bad is None, f"{what}: {bad}"
    return arena.words


# ------------------------------------------------------------------------------------------------------------------------------------------------------
# Adam
# ------------------------------------------------------------------------------------------------------------------------------------------------------
def _adam_multi(arena, t, hp, step, gscale):
    from dcvgan_amd.native import check, stream_ptr
    check(_lib().dcv_adam_step_multi(len(arena.sizes), _ptrs(t["p"], arena), _ptrs(t["g"], arena), _ptrs(t["m"], arena), _ptrs(t["v"], arena), _numel(arena),
                                     *hp, step, gscale, stream_ptr()), "dcv_adam_step_multi")


def _adam_single(arena, t, hp, step, gscale):
    from dcvgan_amd.native import check, stream_ptr
    for s, n in zip(arena.start, arena.sizes):
        a = [C.c_void_p(t[k].data_ptr() + 4 * s) for k in "pgmv"]
        check(_lib().dcv_adam_step(*a, n, *hp, step, gscale, stream_ptr()), "dcv_adam_step")


def _adam_check(arena, call, p, g, m, v, hp, gscale, what, steps=3, single=False, first_step=1):
    """`steps` consecutive steps from (p, g, m, v); the gradient moves on between steps (rolled by one position).  -> compared words"""
    t = {k: _dev(arena.fill(x)) for k, x in zip("pgmv", (p, g, m, v))}
    words = 0
    for step in range(first_step, first_step + steps):
        call(arena, t, hp, step, gscale)
        p, m, v = E.adam_update(p, g, m, v, E.adam_scalars(*hp, step, gscale))
        for k, x in (("m", m), ("v", v), ("p", p)):      # in the update's order: the first to differ names the operation
            bad = E.first_mismatch(arena, _host(t[k]), arena.fill(x))
            if bad is not None and single:
                w = int(np.nonzero(_host(t[k]).view(U32) != arena.fill(x).view(U32))[0][0])
                loc = arena.locate(w)
                bad += "" if loc is None else " | " + E.describe_single(arena.sizes[loc[0]], loc[1])
            assert bad is None, f"{what} step {step}: {k} differs first ({ {'m': 'lerp', 'v': 'addcmul', 'p': 'sqrt / divide tail'}[k]}): {bad}"
            words += arena.words
        assert E.first_mismatch(arena, _host(t["g"]), arena.fill(g)) is None, f"{what}: the gradient was written"
        g = np.roll(g, 1)
        t["g"] = _dev(arena.fill(g))
    return words


@pytest.mark.parametrize("name", list(E.LISTS))
def test_adam_multi(name):
    sizes = E.LISTS[name]
    arena = E.Arena(sizes)
    words = cases = 0
    for nz in (False, True):
        p, g, m, v = E.adam_case(sizes, E.MT * len(sizes) + nz, nz)
        for hp_name, hp in HPS.items():
            for gscale in GSCALES:
                words += _adam_check(arena, _adam_multi, p, g, m, v, hp, gscale, f"adam_multi {name} {hp_name} gscale {gscale:.3g} state {'random' if nz else 'zero'}")
                cases += 1
    _tally("adam_multi", cases, words)


def test_adam_single():
    """dcv_adam_step on every tensor of `ragged` (n = 1, 255, 257 among them), tensors 5 and 12 four bytes off a 16-byte boundary"""
    sizes = E.RAGGED
    arena = E.Arena(sizes, off=(5, 12))
    words = cases = 0
    for nz in (False, True):
        p, g, m, v = E.adam_case(sizes, 77 + nz, nz)
        for hp_name, hp in HPS.items():
            for gscale in GSCALES:
                words += _adam_check(arena, _adam_single, p, g, m, v, hp, gscale, f"adam_single {hp_name} gscale {gscale:.3g} state {'random' if nz else 'zero'}", single=True)
                cases += 1
    _tally("adam_single", cases, words)


def test_adam_single_grid_stride_second_trip():
    """n = 8192 * 256 + 1: the last element is the first of the grid-stride loop's second trip"""
    n = E.GRID_CAP * E.NT + 1
    assert E.adam_grid(n) == (E.GRID_CAP, 2) and E.adam_grid(n - 1) == (E.GRID_CAP, 1)
    arena = E.Arena([n])
    p, g, m, v = E.adam_case([n], 5, True, unique=False)
    words = _adam_check(arena, _adam_single, p, g, m, v, REF_HP, 1.0 / 3.0, "adam_single second trip", single=True, first_step=7)
    _tally("adam_single", 1, words)


@pytest.mark.parametrize("entry", ["multi", "single"])
def test_adam_denormals(entry):
    """|g| around 1e-20 (g g and w2 g g denormal) and 1e-23 (both zero); v from 0 and from 1e-40; a p element at 0 with weight decay on"""
    sizes = [1, 5, 257, 4097, 3]
    arena = E.Arena(sizes, off=(2,) if entry == "single" else ())
    rng = np.random.default_rng(31)
    total = sum(sizes)
    p = E.unique_normal(rng, total, 0.05)
    p[[0, 1, 300, 4000]] = 0.0
    g = E.unique_normal(rng, total, E.per_tensor(sizes, [1e-20, 1e-23, 1e-20, 1e-23, 1e-20]))
    call = _adam_multi if entry == "multi" else _adam_single
    words = 0
    for v0 in (0.0, 1e-40):
        v = np.full(total, v0, F32)
        if v0:
            v = (v * (1 + np.arange(total) % 5)).astype(F32)
        m = np.zeros(total, F32)
        g2 = (g.astype(F64) * g.astype(F64)).astype(F32)
        assert (g2[:1] != 0).all() and (np.abs(g2[:1]) < 2.0 ** -126).all() and (g2[1:6] == 0).all()
        words += _adam_check(arena, call, p, g, m, v, REF_HP, 1.0, f"adam {entry} denormal v0 {v0}", single=entry == "single")
    _tally("adam_denormal", 2, words)


def test_adam_against_torch_on_the_device():
    """The existing 1e-6 max-relative bar against torch.optim.Adam(foreach=False, fused=False) on the device, `ragged`, 10 steps — and, for the record only, the number of
    words that differ (tests/golden/opt_exact_notes.json)."""
    sizes = E.RAGGED
    arena = E.Arena(sizes)
    p, g, m, v = E.adam_case(sizes, 11, False)
    t = {k: _dev(arena.fill(x)) for k, x in zip("pgmv", (p, g, m, v))}
    params = [torch.nn.Parameter(torch.from_numpy(x.copy()).to(DEV)) for x in arena.split(p)]
    opt = torch.optim.Adam(params, lr=REF_HP[0], betas=REF_HP[1:3], eps=REF_HP[3], weight_decay=REF_HP[4], foreach=False, fused=False)
    for step in range(1, 11):
        for q, x in zip(params, arena.split(g)):
            q.grad = torch.from_numpy(x.copy()).to(DEV)
        opt.step()
        _adam_multi(arena, t, REF_HP, step, 1.0)
        g = np.roll(g, 1)
        t["g"] = _dev(arena.fill(g))
    torch.cuda.synchronize()
    diff = {}
    for key, theirs in (("p", [q.detach() for q in params]), ("m", [opt.state[q]["exp_avg"] for q in params]), ("v", [opt.state[q]["exp_avg_sq"] for q in params])):
        mine = arena.split(arena.gather(_host(t[key])))
        diff[key] = 0
        for a, b in zip(mine, theirs):
            b = _host(b)
            diff[key] += int((a.view(U32) != b.view(U32)).sum())
            assert float(np.abs(a.astype(F64) - b.astype(F64)).max() / np.abs(b.astype(F64)).max()) <= 1e-6, key
    print(f"\n[adam vs torch on the device] ragged, 10 steps, {arena.total} elements: differing words p {diff['p']} m {diff['m']} v {diff['v']} (informational)")


# ------------------------------------------------------------------------------------------------------------------------------------------------------
# the gradient guard
# ------------------------------------------------------------------------------------------------------------------------------------------------------
WS_BAND = 64      # bytes of 0xA5 on either side of the workspace


def _state(loss_scale=1.0, tracker=0.0, skipped_total=0.0):
    st = np.zeros(8, F32)
    st[E.LOSS_SCALE], st[E.GROWTH_TRACKER], st[E.SKIPPED_TOTAL] = loss_scale, tracker, skipped_total
    return st


def _measure(arena, gt, rule, state_t):
    """one dcv_grad_guard_measure with a caller-owned workspace -> (partials, counts) as the kernel laid them out; the workspace's bands and its unused tail are checked"""
    from dcvgan_amd.native import check, stream_ptr
    lib = _lib()
    nb = E.total_blocks(arena.sizes)
    ws_bytes = lib.dcv_grad_guard_workspace_bytes(C.c_int64(arena.total), len(arena.sizes))
    assert ws_bytes >= 12 * nb
    ws = torch.full((ws_bytes + 2 * WS_BAND,), 0xA5, dtype=torch.uint8, device=DEV)
    check(lib.dcv_grad_guard_measure(len(arena.sizes), _ptrs(gt, arena), _numel(arena), rule.grad_scale, rule.max_norm, rule.skip_nonfinite, rule.dynamic,
                                     rule.growth, rule.backoff, rule.growth_interval, C.c_void_p(state_t.data_ptr()), C.c_void_p(ws.data_ptr() + WS_BAND), ws_bytes,
                                     stream_ptr()), "dcv_grad_guard_measure")
    raw = _host(ws)
    body = raw[WS_BAND:WS_BAND + ws_bytes]
    assert (raw[:WS_BAND] == 0xA5).all() and (raw[WS_BAND + ws_bytes:] == 0xA5).all() and (body[12 * nb:] == 0xA5).all(), "the guard wrote outside its nb doubles and nb counts"
    return body[:8 * nb].copy().view(F64), body[8 * nb:12 * nb].copy().view(U32)


def _bits_equal(a, b, view):
    """bit for bit, a NaN matching any NaN (the payload a device NaN carries is not specified)"""
    a, b = np.asarray(a), np.asarray(b)
    return (a.view(view) == b.view(view)) | (np.isnan(a) & np.isnan(b))


def _guard_check(arena, g, rule, state, what, aligned=None, state_t=None):
    """measure on the device, mirror on the host, compare every partial, every count and the eight state floats -> (partials, state after, words)"""
    gt = _dev(arena.fill(g))
    state_t = _dev(state) if state_t is None else state_t
    part, cnt = _measure(arena, gt, rule, state_t)
    al = [o == 0 for o in arena.off] if aligned is None else aligned
    wp, wc = E.guard_partials(arena.split(g), al)
    owners = E.block_owner(arena.sizes)
    okp, okc = _bits_equal(part, wp, U64), cnt == wc
    for i in np.nonzero(~(okp & okc))[0][:1]:
        k, slot, t, blk, idx = owners[i]
        raise AssertionError(f"{what}: partial {idx} (table {k} slot {slot}, tensor {t} n = {arena.sizes[t]}, its block {blk}): got {part[i]!r} / {cnt[i]} want {wp[i]!r} / {wc[i]}")
    want = E.guard_decide(wp, wc, rule, state)
    got = _host(state_t)
    assert _bits_equal(got, want, U32).all(), f"{what}: state {got.tolist()} want {want.tolist()}"
    assert E.first_mismatch(arena, _host(gt), arena.fill(g)) is None, f"{what}: the gradient was written"
    return part, got, 3 * len(part) + 8


GUARD_RULE = E.Rule(grad_scale=1.0, max_norm=1.0)


@pytest.mark.parametrize("base", ["aligned", "off"])
@pytest.mark.parametrize("name", list(E.LISTS))
def test_guard_integer_sums(name, base):
    """gradients +-{1..15} times a power of two per tensor, sum of squares below 2^22: every partial is an exact integer multiple of 2^-6 and one element more or less
    moves the fp32 norm; tensors 6, 16 and 26 (or the last) four bytes off in the `off` form"""
    sizes = E.LISTS[name]
    arena = E.Arena(sizes, off=E.guard_offs(sizes) if base == "off" else ())
    g = E.guard_int_case(sizes, E.MT + len(sizes))
    part, st, words = _guard_check(arena, g, GUARD_RULE, _state(), f"guard integer {name} {base}")
    want = [float((x[b * 4096:(b + 1) * 4096].astype(F64) ** 2).sum()) for x in arena.split(g) for b in range(E.mt_blocks(x.size))]
    assert part.tolist() == want
    assert st[E.GRAD_NORM] == F32(np.sqrt(sum(want))) and st[E.NONFINITE] == 0
    _tally("guard_integer", 1, words)


def _real_case(name):
    sizes = E.LISTS[name]
    rng = np.random.default_rng(len(sizes))
    return sizes, E.unique_normal(rng, sum(sizes), E.per_tensor(sizes, 10.0 ** -(np.arange(len(sizes)) % 4).astype(F64)))


@pytest.mark.parametrize("name", ["ragged", "counts49"])
def test_guard_real_values_against_the_mirror(name):
    sizes, g = _real_case(name)
    _, _, words = _guard_check(E.Arena(sizes), g, GUARD_RULE, _state(), f"guard real {name}")
    _tally("guard_real", 1, words)


@pytest.mark.parametrize("name", ["ragged", "counts49"])
def test_guard_alignment_independence(name):
    """the same values at aligned bases and with tensors 6, 16, 26 (or the last) four bytes off: identical partials and state words (guard_partial_kernel's MT_QUAD_ORDER)"""
    sizes, g = _real_case(name)
    off = E.Arena(sizes, off=E.guard_offs(sizes) + [i for i in (23, 24) if i < len(sizes)])      # (counts49: its two ragged tensors as well, the others have 1 .. 7 elements)
    assert any(o and n > 4096 for o, n in zip(off.off, sizes))
    pa, sa, _ = _guard_check(E.Arena(sizes), g, GUARD_RULE, _state(), f"guard real {name} aligned")
    po, so, words = _guard_check(off, g, GUARD_RULE, _state(), f"guard real {name}, three tensors 4 bytes off", aligned=[True] * len(sizes))
    assert np.array_equal(pa.view(U64), po.view(U64)) and np.array_equal(sa.view(U32), so.view(U32))
    _tally("guard_alignment", 1, words)


def _payload_nan():
    return np.array([0x7fc12345], U32).view(F32)[0]


NONFINITE_CASES = {
    # name: (list, [(tensor, element, value)], {partial index: count})
    "ragged_tail_last": ("ragged", [(13, 4096, np.inf)], None),
    "elements_4095_4096": ("ragged", [(14, 4095, -np.inf), (14, 4096, _payload_nan())], None),
    "table_edge": ("counts49", [(23, 4096, _payload_nan()), (24, 0, np.inf), (24, 8192, -np.inf)], None),
    "one_thread_all_three": ("ragged", [(12, 0, np.inf), (12, 1, -np.inf), (12, 2, _payload_nan())], None),
}


@pytest.mark.parametrize("base", ["aligned", "off"])
@pytest.mark.parametrize("case", list(NONFINITE_CASES))
def test_guard_nonfinite(case, base):
    name, plants, _ = NONFINITE_CASES[case]
    sizes = E.LISTS[name]
    arena = E.Arena(sizes, off=E.guard_offs(sizes) + [t for t, _, _ in plants] if base == "off" else ())
    g = E.guard_int_case(sizes, 3)
    for t, e, val in plants:
        assert e < sizes[t]
        g[arena.first[t] + e] = val
    words = 0
    for order in ((0, 1), (1, 1), (1, 0)):
        state_t, state = _dev(_state(loss_scale=1024.0)), _state(loss_scale=1024.0)
        for i, skip in enumerate(order):
            rule = E.Rule(max_norm=1.0, skip_nonfinite=skip)
            part, st, w = _guard_check(arena, g, rule, state, f"guard nonfinite {case} {base} skip_nonfinite {skip}", state_t=state_t)
            words += w
            state = st
            assert st[E.NONFINITE] == len(plants) and st[E.SKIPPED] == skip and st[E.SKIPPED_TOTAL] == sum(order[:i + 1]) and st[E.CLIP_COEF] == 1.0
        # the counts sit in the blocks that own the planted elements, and nowhere else
        _, cnt = _measure(arena, _dev(arena.fill(g)), rule, _dev(_state()))
        want = np.zeros(len(cnt), U32)
        tabs = E.tables(sizes)
        for t, e, _ in plants:
            tab = tabs[t // E.MT]
            want[tab.block0 + tab.first_block[t % E.MT] + e // E.MT_BLOCK] += 1
        assert np.array_equal(cnt, want), (cnt.nonzero(), want.nonzero())
    _tally("guard_nonfinite", 6, words)


def test_guard_decide():
    """max_norm below, at and above the norm; grad_scale 0.125; a loss scale of 1024; the scaler's growth, back-off and tracker; a growth that would overflow"""
    sizes, g = _real_case("ragged")
    arena = E.Arena(sizes)
    norm = float(E.guard_decide(*E.guard_partials(arena.split(g)), E.Rule(), _state())[E.GRAD_NORM])
    words = cases = 0
    for gs, scale in ((1.0, 1.0), (0.125, 1.0), (1.0, 1024.0), (0.125, 1024.0)):
        true = norm * gs / scale
        for mx in (0.5 * true, true, 2.0 * true, 0.0):
            _, st, w = _guard_check(arena, g, E.Rule(grad_scale=gs, max_norm=mx), _state(loss_scale=scale), f"guard decide grad_scale {gs} scale {scale} max_norm {mx}")
            assert (st[E.CLIP_COEF] < 1.0) == (0.0 < mx <= true) and st[E.SKIPPED] == 0
            words += w; cases += 1
    # dynamic scaling: growth_interval 2, five measurements, the third non-finite
    bad = g.copy()
    bad[arena.first[9] + 1000] = np.inf
    rule = E.Rule(max_norm=0.5 * norm / 1024, dynamic=1, growth=2.0, backoff=0.5, growth_interval=2)
    state_t, state, seen = _dev(_state(loss_scale=1024.0)), _state(loss_scale=1024.0), []
    for i, x in enumerate((g, g, bad, g, g)):
        _, state, w = _guard_check(arena, x, rule, state, f"guard scaler measurement {i}", state_t=state_t)
        seen.append((float(state[E.LOSS_SCALE]), float(state[E.GROWTH_TRACKER]), float(state[E.SKIPPED]), float(state[E.SKIPPED_TOTAL])))
        words += w; cases += 1
    assert seen == [(1024, 1, 0, 0), (2048, 0, 0, 0), (1024, 0, 1, 1), (1024, 1, 0, 1), (2048, 0, 0, 1)], seen
    _, st, w = _guard_check(arena, g, E.Rule(dynamic=1, growth=2.0, backoff=0.5, growth_interval=1), _state(loss_scale=3e38), "guard scaler overflowing growth")
    assert st[E.LOSS_SCALE] == F32(3e38) and st[E.GROWTH_TRACKER] == 0
    _tally("guard_decide", cases + 1, words + w)


# ------------------------------------------------------------------------------------------------------------------------------------------------------
# the guarded Adam
# ------------------------------------------------------------------------------------------------------------------------------------------------------
def _adam_guarded(arena, t, hp, block_t, state_t):
    from dcvgan_amd.native import check, stream_ptr
    check(_lib().dcv_adam_step_multi_guarded(len(arena.sizes), _ptrs(t["p"], arena), _ptrs(t["g"], arena), _ptrs(t["m"], arena), _ptrs(t["v"], arena), _numel(arena),
                                             *hp, C.c_void_p(block_t.data_ptr()), C.c_void_p(state_t.data_ptr()), stream_ptr()), "dcv_adam_step_multi_guarded")


@pytest.mark.parametrize("name", ["counts25"] + [k for k in E.LISTS if k.startswith("zeros_")])
def test_adam_guarded(name):
    """three guarded steps after three measurements, the second of them non-finite and skipped"""
    sizes = E.LISTS[name]
    arena = E.Arena(sizes)
    p, g, m, v = E.adam_case(sizes, 5 + len(sizes), True)
    bad = g.copy()
    bad[-1] = np.inf
    t = {k: _dev(arena.fill(x)) for k, x in zip("pmv", (p, m, v))}
    block_t, state_t, state = torch.zeros(16, dtype=torch.int32, device=DEV), _dev(_state()), _state()
    norm = float(E.guard_decide(*E.guard_partials(arena.split(g)), E.Rule(), _state())[E.GRAD_NORM])
    rule = E.Rule(grad_scale=0.125, max_norm=0.03 * norm, skip_nonfinite=1)
    words, counts = 0, []
    for i, x in enumerate((g, bad, np.roll(g, 1))):
        t["g"] = _dev(arena.fill(x))
        _, state, w = _guard_check(arena, x, rule, state, f"adam_guarded {name} measurement {i}", state_t=state_t)
        _adam_guarded(arena, t, REF_HP, block_t, state_t)
        blk = _host(block_t)
        counts.append(int(blk[0]))
        if state[E.SKIPPED] == 0:
            k = E.adam_scalars(*REF_HP, int(blk[0]), float(state[E.FACTOR]))
            assert blk[1] == 0 and np.array_equal(blk[2:10].view(F32).view(U32), np.array(k, F32).view(U32)), (blk[2:10].view(F32).tolist(), k)
            p, m, v = E.adam_update(p, x, m, v, k)
        else:
            assert blk[1] == 1
        for key, val in (("m", m), ("v", v), ("p", p)):      # after a skipped call: every word as it was
            words += _same(arena, t[key], arena.fill(val), f"adam_guarded {name} call {i} ({'skipped' if state[E.SKIPPED] else 'applied'}): {key}")
        words += w
    assert counts == [1, 1, 2] and state[E.CLIP_COEF] < 1.0
    _tally("adam_guarded", 1, words)


@pytest.mark.parametrize("betas", [(0.5, 0.999), (0.9, 0.99)], ids=["b.5_.999", "b.9_.99"])
def test_guarded_and_unguarded_scalars_agree(betas):
    """Steps 1 .. 20 on one small tensor: the guarded step (bias corrections formed on the device, pow and sqrt in double) against dcv_adam_step_multi with the same
    step and grad_scale = FACTOR (formed on the host), bit for bit; and the device's scalars against Python's ** and math.sqrt."""
    sizes = [37]
    arena = E.Arena(sizes)
    hp = (REF_HP[0], betas[0], betas[1], REF_HP[3], REF_HP[4])
    p, g, m, v = E.adam_case(sizes, 3, True)
    a = {k: _dev(arena.fill(x)) for k, x in zip("pgmv", (p, g, m, v))}
    b = {k: _dev(arena.fill(x)) for k, x in zip("pgmv", (p, g, m, v))}
    block_t, state_t = torch.zeros(16, dtype=torch.int32, device=DEV), _dev(_state())
    _guard_check(arena, g, E.Rule(grad_scale=1.0 / 3.0, max_norm=0.5), _state(), "scalars: measurement", state_t=state_t)
    factor = float(_host(state_t)[E.FACTOR])
    differ, words = [], 0
    for step in range(1, 21):
        _adam_guarded(arena, a, hp, block_t, state_t)
        _adam_multi(arena, b, hp, step, factor)
        blk = _host(block_t)
        dev_k, host_k = blk[2:10].view(F32), np.array(E.adam_scalars(*hp, step, factor), F32)
        same = all(np.array_equal(_host(a[k]).view(U32), _host(b[k]).view(U32)) for k in "pmv") and np.array_equal(dev_k.view(U32), host_k.view(U32))
        if int(blk[0]) != step or not same:
            differ.append((step, int(blk[0]), dev_k.tolist(), host_k.tolist()))
        words += 3 * arena.words + 8
    print(f"\n[guarded vs unguarded scalars] betas {betas}: steps that differ: {differ if differ else 'none of 20'}")
    assert not differ, differ
    _tally("adam_scalars", 1, words)


# ------------------------------------------------------------------------------------------------------------------------------------------------------
# EMA
# ------------------------------------------------------------------------------------------------------------------------------------------------------
def _ema(arena_e, et, arena_s, st, modes, decay, warmup, block_t, state_t=None, null_empty=False):
    from dcvgan_amd.native import c_array, check, stream_ptr
    check(_lib().dcv_ema_update_multi(len(modes), _ptrs(et, arena_e, null_empty), _ptrs(st, arena_s, null_empty), _numel(arena_e), c_array(modes, C.c_int32), decay, int(warmup),
                                      C.c_void_p(block_t.data_ptr()), None if state_t is None else C.c_void_p(state_t.data_ptr()), stream_ptr()), "dcv_ema_update_multi")


EMA_FORMS = ("aligned", "both_off", "source_off", "ema_off")


@pytest.mark.parametrize("name", list(E.LISTS))
def test_ema(name):
    """five updates with changing sources, in four alignment forms (every odd tensor off, on both sides, the source's only or the EMA's only); copied tensors in
    slots 2 and 5 of the first table and in slots 0 and 23 of the second"""
    sizes = E.LISTS[name]
    nt = len(sizes)
    odd = [i for i in range(nt) if i % 2]
    modes = [1 if i in (2, 5, 24, 47) else 0 for i in range(nt)]
    copied = np.repeat(np.array(modes, bool), sizes)
    words = cases = 0
    runs = [(f, 0.999, True, False) for f in EMA_FORMS] + [("aligned", 0.9, False, False)]
    if 0 in sizes:
        runs.append(("aligned", 0.999, True, True))      # NULL pointers for the zero-element tensors
    for form, decay, warmup, null_empty in runs:
        ae = E.Arena(sizes, off=odd if form in ("both_off", "ema_off") else ())
        as_ = E.Arena(sizes, off=odd if form in ("both_off", "source_off") else ())
        rng = np.random.default_rng(nt + len(form))
        e = E.unique_normal(rng, sum(sizes), 3.0)
        et, block_t = _dev(ae.fill(e)), torch.zeros(16, dtype=torch.int32, device=DEV)
        for t in range(5):
            s = E.unique_normal(rng, sum(sizes), 2.0 + t)
            s[copied] = np.arange(int(copied.sum()), dtype=U32).view(F32) if t == 0 else s[copied]      # copy mode moves bit patterns: denormal words in the first update
            st = _dev(as_.fill(s))
            _ema(ae, et, as_, st, modes, decay, warmup, block_t, null_empty=null_empty)
            e = np.where(copied, s, E.ema_update(e, s, E.ema_w(t, decay, warmup)))
            what = f"ema {name} {form} decay {decay} warm-up {warmup} null {null_empty} update {t}"
            words += _same(ae, et, ae.fill(e), what, E.STRIDED if form != "aligned" else E.QUAD)
            assert E.first_mismatch(as_, _host(st), as_.fill(s)) is None, what + ": the source was written"
            assert int(_host(block_t)[0]) == t + 1
        cases += 1
    _tally("ema", cases, words)


@pytest.mark.parametrize("warmup", [True, False], ids=["warmup", "no_warmup"])
def test_ema_weight_count_and_skip(warmup):
    """w read through e = 0, s = 1 (fmaf(w, 1 - 0, 0) = w) for updates 0 .. 11; the count; and a guard-skipped update, which changes no word and no count"""
    arena = E.Arena([1])
    st_ = _dev(arena.fill(np.ones(1, F32)))
    block_t = torch.zeros(16, dtype=torch.int32, device=DEV)
    skip, go = _state(), _state()
    skip[E.SKIPPED] = 1.0
    skip_t, go_t = _dev(skip), _dev(go)
    for t in range(12):
        et = _dev(arena.fill(np.zeros(1, F32)))
        _ema(arena, et, arena, st_, [0], 0.999, warmup, block_t, state_t=skip_t)
        _same(arena, et, arena.fill(np.zeros(1, F32)), f"ema skipped update {t}")
        blk = _host(block_t)
        assert int(blk[0]) == t and int(blk[1]) == 1
        _ema(arena, et, arena, st_, [0], 0.999, warmup, block_t, state_t=go_t if t % 2 else None)
        w = E.ema_w(t, 0.999, warmup)
        _same(arena, et, arena.fill(np.array([w], F32)), f"ema weight of update {t}")
        blk = _host(block_t)
        assert int(blk[0]) == t + 1 and int(blk[1]) == 0 and blk[2:3].view(U32)[0] == np.array([w], F32).view(U32)[0]
    _tally("ema_weight", 1, 12 * 2 * arena.words)
