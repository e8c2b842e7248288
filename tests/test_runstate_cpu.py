"""CPU: RunState's digest mirror, manifest, the optimiser / guard / random-stream checkpoints and the file checks.

`digest_host` is the specification tests/test_runstate_gpu.py holds the kernels to; here it is checked against a scalar restatement in Python integers."""
import copy
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import rig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dcv_state_workspace_bytes", "dcv_state_pack_multi", "dcv_state_unpack_multi", "dcv_state_digest_multi")
M64 = (1 << 64) - 1
CPU = torch.device("cpu")


def digest_scalar(words):
    """The issue's definition, one dword at a time, in Python integers."""
    s = x = 0
    for i, w in enumerate(int(v) for v in words):
        z = (i * 0x9E3779B97F4A7C15 + w) & M64
        z ^= z >> 30
        z = (z * 0xBF58476D1CE4E5B9) & M64
        z ^= z >> 27
        z = (z * 0x94D049BB133111EB) & M64
        z ^= z >> 31
        s = (s + z) & M64
        x ^= z
    return s, x


def _cases():
    g = np.random.default_rng(3)
    nan = np.array([0x7FC00001, 0xFFC12345, 0x7F800001, 0x7FC00000], dtype=np.uint32).view(np.float32)
    return [
        np.zeros(0, dtype=np.float32),
        np.array([1.5], dtype=np.float32),
        np.array([3, -1, 1 << 40, -(1 << 62)], dtype=np.int64),
        nan,
        np.array([-0.0, 0.0, -0.0], dtype=np.float32),
        np.array([np.inf, -np.inf, 1e-45], dtype=np.float32),
        g.standard_normal(4097).astype(np.float32),
        g.integers(-2 ** 31, 2 ** 31, size=257).astype(np.int32),
        g.standard_normal(33),                                   # float64: two dwords per element
        g.standard_normal((5, 7)).astype(np.float32).T,          # not contiguous: the digest is of the logical row-major order
        np.float32(2.25),                                        # 0-d
        np.zeros(300, dtype=np.int32),
        np.full(5, -1, dtype=np.int32),
    ]


def test_digest_host_equals_the_scalar_restatement():
    from dcvgan_amd import runstate as RS
    seen = set()
    for k, a in enumerate(_cases()):
        words = np.ascontiguousarray(a).reshape(-1).view(np.uint32)
        want = digest_scalar(words)
        assert RS.digest_host(a) == want, k
        assert RS.digest_host(torch.from_numpy(np.ascontiguousarray(a))) == want, k
        seen.add(want)
    assert RS.digest_host(np.zeros(0, dtype=np.float32)) == (0, 0)
    assert len(seen) == len(_cases())
    # NaN payloads and the sign of zero are bits like any other
    assert RS.digest_host(np.array([0.0], np.float32)) != RS.digest_host(np.array([-0.0], np.float32))
    a, b = np.array([0x7FC00000], np.uint32).view(np.float32), np.array([0x7FC00001], np.uint32).view(np.float32)
    assert RS.digest_host(a) != RS.digest_host(b)
    for bad in (np.zeros(3, dtype=np.float16), np.zeros(4, dtype=np.uint8), torch.zeros(2, dtype=torch.bfloat16)):
        with pytest.raises(RS.NativeError, match="32-bit words"):
            RS.digest_host(bad)


def test_digest_is_sensitive_to_value_and_position():
    from dcvgan_amd import runstate as RS
    base = np.arange(1, 41, dtype=np.uint32) * np.uint32(2654435761)
    d0 = RS.digest_host(base)
    for i, bit in ((0, 0), (7, 31), (39, 13)):      # a single-bit flip
        a = base.copy()
        a[i] ^= np.uint32(1 << bit)
        d = RS.digest_host(a)
        assert d[0] != d0[0] and d[1] != d0[1], (i, bit)
    for i, j in ((0, 1), (3, 38)):                  # a swap of two unequal elements
        a = base.copy()
        a[i], a[j] = base[j], base[i]
        d = RS.digest_host(a)
        assert d[0] != d0[0] and d[1] != d0[1], (i, j)
    sparse = np.zeros(16, dtype=np.uint32)
    sparse[2] = 77
    moved = np.zeros(16, dtype=np.uint32)
    moved[9] = 77                                   # the same value at another index
    assert RS.digest_host(sparse) != RS.digest_host(moved)
    assert RS.digest_host(np.zeros(16, np.uint32)) != RS.digest_host(np.zeros(17, np.uint32))      # the length counts: h(i, 0) != 0


# ---- the binding ------------------------------------------------------------------------------------------------------------------------------------------
def test_new_names_are_bound_declared_and_exported():
    from dcvgan_amd import native
    if not os.path.exists(native.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dcvgan_hip.h")).read(), flags=re.S)
    raw = ctypes.CDLL(native.LIB_PATH)
    for n in NEW:
        assert n in native.EXPORTS, n
        assert re.search(r"\b%s\s*\(" % n, header), f"{n} is not declared in dcvgan_hip.h"
        assert hasattr(raw, n), f"{n} is not exported by the library"
    build = open(os.path.join(ROOT, "dcvgan_amd", "csrc", "build.sh")).read()
    assert re.search(r"for f in [^;]*\brunstate\b", build) and "$OBJ/runstate.o" in build
    assert native.lib().dcv_version() == native.ABI_VERSION == 4


def test_entry_points_refuse_before_any_launch():
    """No GPU is needed to be refused: sizes out of range, misaligned tensors and arenas, overlapping segments, a small workspace."""
    from dcvgan_amd import native
    L = native.lib()
    i64 = lambda xs: (ctypes.c_int64 * len(xs))(*xs)
    vp = lambda xs: (ctypes.c_void_p * len(xs))(*xs)
    n0 = native.launch_count()
    assert L.dcv_state_workspace_bytes(2, i64([4096, 4097])) == 3 * 16
    assert L.dcv_state_workspace_bytes(1, i64([1 << 32])) == 0 and L.dcv_state_workspace_bytes(1, i64([-1])) == 0
    ok = dict(src=vp([0x1000, 0x2004]), dw=i64([5, 3]), arena=ctypes.c_void_p(0x10000), off=i64([0, 8]), dig=ctypes.c_void_p(0x20000), ws=ctypes.c_void_p(0x30000))
    call = lambda **kw: (lambda a: L.dcv_state_pack_multi(2, a["src"], a["dw"], a["arena"], a.get("total", 12), a["off"], a["dig"], a["ws"], a.get("wsb", 32), None))({**ok, **kw})
    assert call(dw=i64([5, 1 << 32])) == native.DCV_EINVAL
    assert call(src=vp([0x1002, 0x2004])) == native.DCV_EINVAL                 # not on a 4-byte boundary
    assert call(arena=ctypes.c_void_p(0x10008)) == native.DCV_EINVAL           # the arena: 16 bytes
    assert call(off=i64([0, 6])) == native.DCV_EINVAL                          # offsets: multiples of 4 dwords
    assert call(off=i64([0, 4])) == native.DCV_EINVAL                          # inside the first segment's padding
    assert call(off=i64([8, 0])) == native.DCV_EINVAL                          # ascending
    assert call(total=11) == native.DCV_EINVAL                                 # the last segment's padding ends outside
    assert call(wsb=31) == native.DCV_EWORKSPACE
    assert b"dcv_state_workspace_bytes" in L.dcv_last_error()
    assert L.dcv_state_unpack_multi(2, ok["src"], ok["dw"], ok["arena"], 12, i64([0, 4]), None) == native.DCV_EINVAL
    assert L.dcv_state_digest_multi(2, vp([0x1000, 0]), ok["dw"], ok["dig"], ok["ws"], 32, None) == native.DCV_EINVAL      # a null tensor with dwords
    assert L.dcv_state_digest_multi(2, ok["src"], ok["dw"], ctypes.c_void_p(0x20004), ok["ws"], 32, None) == native.DCV_EINVAL
    assert native.launch_count() == n0


# ---- the pieces' own checkpoints --------------------------------------------------------------------------------------------------------------------------
def _params(seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(s, generator=g)) for s in ((3, 4), (5,), (2, 3, 2))]


def _torch_adam_after_steps(ps, steps=3):
    ref = torch.optim.Adam(ps, lr=2e-4, betas=(0.5, 0.999), eps=1e-8, weight_decay=1e-5)
    g = torch.Generator().manual_seed(11)
    for _ in range(steps):
        for p in ps[:2]:                     # the third parameter never gets a gradient: it has no state
            p.grad = torch.randn(p.shape, generator=g)
        ref.step()
    return ref


def _same_optimizer_state(a, b):
    assert list(a["state"]) == list(b["state"]) and len(a["param_groups"]) == len(b["param_groups"]) == 1
    for i in a["state"]:
        assert sorted(a["state"][i]) == sorted(b["state"][i]) == ["exp_avg", "exp_avg_sq", "step"]
        assert float(a["state"][i]["step"]) == float(b["state"][i]["step"])
        for k in ("exp_avg", "exp_avg_sq"):
            assert a["state"][i][k].shape == b["state"][i][k].shape and torch.equal(a["state"][i][k], b["state"][i][k])
    ga, gb = a["param_groups"][0], b["param_groups"][0]
    assert sorted(ga) == sorted(gb)
    for k in ("lr", "eps", "weight_decay", "params", "amsgrad", "maximize"):
        assert ga[k] == gb[k], k
    assert tuple(ga["betas"]) == tuple(gb["betas"])


def test_adam_state_dict_is_torch_adams():
    from dcvgan_amd import optim
    ps = _params()
    ref = _torch_adam_after_steps(ps)
    want = ref.state_dict()
    assert sorted(want["state"]) == [0, 1]
    mine = optim.Adam(ps, lr=1.0, betas=(0.9, 0.9), eps=1.0, weight_decay=0.5)
    mine.load_state_dict(want)                        # torch -> here
    assert (mine.lr, mine.betas, mine.eps, mine.weight_decay) == (2e-4, (0.5, 0.999), 1e-8, 1e-5)
    assert [mine.state[p]["step"] for p in ps[:2]] == [3, 3] and ps[2] not in mine.state
    got = mine.state_dict()
    _same_optimizer_state(got, want)
    assert sorted(got["param_groups"][0]) == sorted(want["param_groups"][0])      # the same keys as this torch's Adam writes
    assert got["state"][0]["exp_avg"].data_ptr() != mine.state[ps[0]]["exp_avg"].data_ptr()      # clones
    other = torch.optim.Adam(ps, lr=1.0)
    other.load_state_dict(copy.deepcopy(got))         # here -> torch (which adopts the tensors it is given)
    _same_optimizer_state(other.state_dict(), want)
    back = optim.Adam(ps)
    back.load_state_dict(other.state_dict())          # and back
    _same_optimizer_state(back.state_dict(), got)
    # torch goes on from it exactly as the optimiser it came from
    for p in ps[:2]:
        p.grad = torch.ones_like(p)
    before = [p.detach().clone() for p in ps]
    ref.step()
    after_ref = [p.detach().clone() for p in ps]
    with torch.no_grad():
        for p, b in zip(ps, before):
            p.copy_(b)
    other.step()
    assert all(torch.equal(p, a) for p, a in zip(ps, after_ref))
    # refusals change nothing
    bad = copy.deepcopy(got)
    bad["state"][1]["exp_avg"] = torch.zeros(6)
    with pytest.raises(ValueError, match="exp_avg of parameter 1"):
        back.load_state_dict(bad)
    bad = copy.deepcopy(got)
    bad["param_groups"][0]["amsgrad"] = True
    with pytest.raises(ValueError, match="amsgrad"):
        back.load_state_dict(bad)
    _same_optimizer_state(back.state_dict(), got)
    # a data-parallel wrapper hands over its inner optimiser's
    wrapped = optim.DataParallelAdam(optim.Adam(ps))
    wrapped.load_state_dict(got)
    _same_optimizer_state(wrapped.state_dict(), got)


def test_guarded_adam_state_dict_keeps_the_counts_in_blocks():
    from dcvgan_amd import optim
    ps = _params()
    want = _torch_adam_after_steps(ps).state_dict()
    want["state"][1]["step"] = torch.tensor(7.0)      # a parameter that joined earlier: its own block
    guard = optim.GradGuard(max_norm=1.0)
    mine = optim.Adam(ps, guard=guard)
    mine.load_state_dict(want)
    s0, s1 = mine.state[ps[0]], mine.state[ps[1]]
    assert s0["step_block"].dtype == torch.int32 and s0["step_block"].tolist() == [3] + [0] * 15 and s1["step_block"].tolist() == [7] + [0] * 15
    assert s0["step"].data_ptr() == s0["step_block"].data_ptr() and s0["step_block"].data_ptr() != s1["step_block"].data_ptr()
    _same_optimizer_state(mine.state_dict(), want)


def test_philox_and_guard_round_trips():
    from dcvgan_amd import optim
    from dcvgan_amd.augment import ClipAugment
    from dcvgan_amd.configs import CONFIGS
    from dcvgan_amd.rng import PhiloxRng
    r = PhiloxRng(5)
    for _ in range(3):
        r._next()
    sd = r.state_dict()
    assert sd == dict(fixed_seed=5, seed_seen=5, counter=3)
    q = PhiloxRng()
    q.load_state_dict(sd)
    assert q.state_dict() == sd and q._next() == r._next() == (5, 4)
    free = PhiloxRng()
    torch.manual_seed(1234)
    free._next(); free._next()
    assert free.state_dict() == dict(fixed_seed=None, seed_seen=1234, counter=2)
    q.load_state_dict(free.state_dict())
    assert q._next() == (1234, 3)
    with pytest.raises(ValueError):
        q.load_state_dict(dict(fixed_seed=None, seed_seen=None, counter=-1))
    # the three fields ClipAugment.state_dict() writes by hand are these
    aug = ClipAugment(CONFIGS["isogd-depth"].scaled(batchsize=2, width_div=8), CPU, seed=3)
    assert aug.rng.state_dict() == dict(fixed_seed=3, seed_seen=None, counter=0)
    assert sorted(aug.rng.state_dict()) == ["counter", "fixed_seed", "seed_seen"]

    g = optim.GradGuard(max_norm=2.5, dynamic=True, loss_scale=1024.0, growth_interval=7, backoff_factor=0.25)
    g.measurements = 9
    sd = g.state_dict()
    assert sd["state"] is None and sd["measurements"] == 9 and sd["max_norm"] == 2.5 and sd["init_scale"] == 1024.0
    h = optim.GradGuard()
    h.load_state_dict(sd)
    assert h.state_dict() == sd and (h.dynamic, h.growth_interval, h.backoff_factor) == (True, 7, 0.25)
    with pytest.raises(optim.NativeError, match="no optimiser"):
        h.load_state_dict(dict(sd, state=torch.zeros(8)))


# ---- the manifest and the files (host models) -------------------------------------------------------------------------------------------------------------
def _host_run(seed, width_div=8, guard=None, options=True, stepped=True):
    """Models, optimisers and every optional component on the host, with Adam state as after `3` steps (made up: nothing trains on the CPU)."""
    from dcvgan_amd import trainer
    cfg = rig.small_cfg(width_div=width_div)
    models, r = rig.seeded_models(cfg, CPU, seed, seed + 100)
    opts = trainer.build_optimizers(cfg, models, guard=guard)
    sn = trainer.build_spectral_norm(cfg, models, opts) if options else None
    if stepped:
        g = torch.Generator().manual_seed(seed + 1)
        for n, o in opts.items():
            sd = o.state_dict()
            for i, p in enumerate(o.params):
                sd["state"][i] = {"step": torch.tensor(3.0), "exp_avg": torch.randn(p.shape, generator=g), "exp_avg_sq": torch.rand(p.shape, generator=g)}
            o.load_state_dict(sd)
    ema = trainer.build_ema(cfg, models, opts) if options else None
    aug = trainer.build_augment(cfg, models, opts, p=0.25, interval=1, seed=seed + 7) if options else None
    lc = trainer.build_lecam(cfg, models, opts, weight=0.3, start=0) if options else None
    extra = {"t_rand_seed": seed, "note": "mine"}
    rs = trainer.build_run_state(cfg, models, opts, ema=ema, spectral=sn, augment=aug, lecam=lc, extra=extra)
    return dict(cfg=cfg, models=models, opts=opts, ema=ema, sn=sn, aug=aug, lc=lc, rs=rs, rng=r, extra=extra)


def _all_bytes(run):
    return {e["name"]: t.detach().reshape(-1).view(torch.uint8).clone() for e, t in zip(run["rs"]._layout().manifest, run["rs"]._layout().tensors)}


def test_manifest_order_offsets_and_total():
    from dcvgan_amd import trainer
    run = _host_run(1, guard=dict(max_norm=10.0))
    rs, models, opts = run["rs"], run["models"], run["opts"]
    man = rs.manifest()
    names = [e["name"] for e in man]
    want = []
    for n in trainer.MODEL_NAMES:
        want += [f"model.{n}.{k}" for k in models[n].state_dict()]
    assert any(k.endswith("weight_u") for k in want) and any(k.endswith("num_batches_tracked") for k in want)      # spectral and BatchNorm buffers are state
    for n in trainer.MODEL_NAMES:
        for i in range(len(opts[n].params)):
            want += [f"optim.{n}.{i}.exp_avg", f"optim.{n}.{i}.exp_avg_sq"]
    want += [f"optim.{n}.step_block.0" for n in trainer.MODEL_NAMES]      # every parameter of an optimiser started together: one block each
    # (host optimisers: the guards hold no device floats, so no guard.<k>.state entry here; tests/test_runstate_gpu.py sees them)
    for n in ("ggen", "cgen"):
        want += [f"ema.{n}.{k}" for k in run["ema"].twins[n].state_dict()]
    want += ["ema_count.ggen", "ema_count.cgen", "augment.state", "lecam.state"]
    assert names == want
    off = 0
    for e, t in zip(man, rs._layout().tensors):
        assert e["offset"] == off and (e["offset"] * 4) % 16 == 0, e
        assert e["dwords"] == t.numel() * t.element_size() // 4 and e["dtype"] == str(t.dtype) and e["shape"] == tuple(t.shape), e
        off += (e["dwords"] + 3) // 4 * 4
    assert off * 4 == rs.arena_bytes()
    nbt = next(e for e in man if e["name"].endswith("num_batches_tracked"))
    assert nbt["dtype"] == "torch.int64" and nbt["dwords"] == 2
    snap = rs.capture()
    assert snap.arena.numel() == rs.arena_bytes() and snap.arena.dtype == torch.uint8 and tuple(snap.digests.shape) == (len(man), 2)
    assert rs.launches_per_capture() == 2 * ((len(man) + 23) // 24)
    # host scalars, kept beside it
    h = snap.host
    assert h["optim"]["idis"]["guarded"] and h["optim"]["idis"]["blocks"][0] == "optim.idis.step_block.0" and h["optim"]["ggen"]["betas"] == (0.5, 0.999)
    assert len(h["guards"]) == 2 and h["guards"][0]["max_norm"] == 10.0 and h["iteration"] is None and h["sampler"] is None
    assert h["extra"] == run["extra"] and h["extra"] is not run["extra"]
    assert h["augment"]["interval"] == 1 and h["lecam"]["weight"] == 0.3 and h["spectral"]["eps"] == 1e-12 and h["ema"] == dict(decay=0.999, warmup=True)
    kinds = [(r["fixed_seed"], r["counter"]) for r in h["rngs"]]
    assert len(kinds) == 4 and kinds[1] == (101, 0) and kinds[3] == (8, 0)      # the process-wide stream, the models', the twins', the augmentation's
    # an unguarded, unstepped run: no optimiser entries at all, and the step counts are host scalars
    bare = _host_run(1, options=False, stepped=False)
    assert not [e for e in bare["rs"].manifest() if not e["name"].startswith("model.")]
    stepped = _host_run(1, options=False)
    assert stepped["rs"].capture().host["optim"]["vdis"]["steps"] == [3] * len(stepped["opts"]["vdis"].params)
    # a 16-bit tensor is refused before anything happens
    stepped["models"]["idis"].register_buffer("fp16_buf", torch.zeros(3, dtype=torch.float16))
    with pytest.raises(trainer.optim.NativeError, match="model.idis.fp16_buf.*32-bit words"):
        stepped["rs"].capture()


def test_rollback_and_file_round_trip_on_the_host(tmp_path):
    from dcvgan_amd import runstate as RS
    a = _host_run(1, guard=dict(max_norm=10.0))
    rs = a["rs"]
    want_bytes, want_fp = _all_bytes(a), rs.fingerprint_host()
    assert list(want_fp) == [e["name"] for e in rs.manifest()]
    for e, t in zip(rs._layout().manifest, rs._layout().tensors):
        assert want_fp[e["name"]] == tuple(RS._signed(RS.digest_host(t)))
    snap = rs.capture()
    path = str(tmp_path / "run.pt")
    snap.save(path)
    # rollback: everything moves, then comes back
    with torch.no_grad():
        for t in rs._layout().tensors:
            t.add_(1)
    versions = [t._version for t in rs._layout().tensors]
    a["rng"]._next(); a["aug"].rng._next()
    a["opts"]["ggen"].lr, a["lc"].weight, a["extra"]["t_rand_seed"] = 9.0, 0.9, -5
    a["extra"]["more"] = 1
    changed = RS.RunState.diff(want_fp, rs.fingerprint_host())
    assert len(changed) == len(want_fp)
    snap.restore()
    assert RS.RunState.diff(want_fp, rs.fingerprint_host()) == []
    got = _all_bytes(a)
    assert all(torch.equal(got[k], want_bytes[k]) for k in want_bytes)
    assert all(t._version > v for t, v in zip(rs._layout().tensors, versions))      # the caches keyed on the version see a change
    assert a["rng"].state_dict()["counter"] == 0 and a["aug"].rng.state_dict()["counter"] == 0
    assert a["opts"]["ggen"].lr == a["cfg"].lr["ggen"] and a["lc"].weight == 0.3 and a["extra"] == {"t_rand_seed": 1, "note": "mine"}
    # resume in fresh objects built from other seeds, with no optimiser state yet
    b = _host_run(2, guard=dict(max_norm=3.0), stepped=False)
    assert RS.RunState.diff(want_fp, b["rs"].fingerprint_host())
    b["rs"].load(path).restore()
    assert RS.RunState.diff(want_fp, b["rs"].fingerprint_host()) == []
    got = _all_bytes(b)
    assert got.keys() == want_bytes.keys() and all(torch.equal(got[k], want_bytes[k]) for k in want_bytes)
    assert b["opts"]["idis"].guard.max_norm == 10.0 and b["rng"].state_dict() == a["rng"].state_dict() and b["extra"] == a["extra"]
    s = b["opts"]["cgen"].state
    blocks = {s[p]["step_block"].data_ptr() for p in b["opts"]["cgen"].params}
    assert len(blocks) == 1 and all(s[p]["step"].data_ptr() in blocks for p in b["opts"]["cgen"].params)
    # a snapshot from before the first step drops the live optimiser's state
    c = _host_run(1, stepped=False)
    early = c["rs"].capture()
    c2 = _host_run(1)
    RS.Snapshot(c2["rs"], early.manifest, early.host, early.arena, early.digests, None).restore()
    assert all(not o.state for o in c2["opts"].values())
    # the model's checkpoint, cut out of the file
    sd = RS.model_state_dict(path, "cgen")
    live = a["models"]["cgen"].state_dict()
    assert list(sd) == list(live) and all(sd[k].dtype == live[k].dtype and torch.equal(sd[k], live[k]) for k in live)
    twin = RS.model_state_dict(path, "ema.ggen")
    assert list(twin) == list(a["ema"].twins["ggen"].state_dict())
    b["models"]["cgen"].load_state_dict(sd)
    with pytest.raises(RS.NativeError, match="no entry"):
        RS.model_state_dict(path, "nobody")
    # the ring: a third capture takes the first one's arena
    s1, s2, s3 = rs.capture(), rs.capture(), rs.capture()
    assert s1.arena is s3.arena and s2.arena is not s3.arena
    with pytest.raises(RS.NativeError, match="overwritten"):
        s1.restore()
    s2.restore(); s3.restore()


def test_damaged_and_foreign_files_are_refused(tmp_path):
    from dcvgan_amd import runstate as RS
    a = _host_run(1)
    path = str(tmp_path / "run.pt")
    a["rs"].capture().save(path)
    f = torch.load(path, weights_only=True)
    assert sorted(f) == ["arena", "digests", "format", "host", "manifest"] and f["format"] == RS.FORMAT_VERSION and f["arena"].dtype == torch.uint8
    victim = next(e for e in f["manifest"] if e["name"].startswith("model.vdis.") and e["dwords"] >= 8)
    before = _all_bytes(a)
    # one arena byte flipped: refused, the entry named
    g = copy.deepcopy(f)
    g["arena"][4 * victim["offset"] + 5] ^= 0x10
    bad = str(tmp_path / "flipped.pt")
    torch.save(g, bad)
    with pytest.raises(RS.NativeError, match=re.escape(victim["name"]) + ".*damaged"):
        a["rs"].load(bad)
    # a flipped padding byte is caught too (num_batches_tracked is two dwords: two dwords of padding follow)
    nbt = next(e for e in f["manifest"] if e["name"].endswith("num_batches_tracked"))
    g = copy.deepcopy(f)
    g["arena"][4 * (nbt["offset"] + 2)] ^= 1
    torch.save(g, bad)
    with pytest.raises(RS.NativeError, match=re.escape(nbt["name"]) + ".*padding"):
        a["rs"].load(bad)
    # another format
    g = copy.deepcopy(f)
    g["format"] = 99
    torch.save(g, bad)
    with pytest.raises(RS.NativeError, match="format 99"):
        a["rs"].load(bad)
    # a file from another width: refused before anything is written, the first differing entry named
    narrow = _host_run(1, width_div=16)
    first = next(e["name"] for e, m in zip(f["manifest"], narrow["rs"].manifest()) if tuple(e["shape"]) != tuple(m["shape"]))
    kept = _all_bytes(narrow)
    with pytest.raises(RS.NativeError, match=re.escape(first)):
        narrow["rs"].load(path)
    now = _all_bytes(narrow)
    assert all(torch.equal(now[k], kept[k]) for k in kept)
    # a run without the optional components does not take a file that has them
    plain = _host_run(1, options=False)
    with pytest.raises(RS.NativeError):
        plain["rs"].load(path)
    now = _all_bytes(a)
    assert all(torch.equal(now[k], before[k]) for k in before)
    assert a["rs"].load(path).manifest == [dict(e, shape=tuple(e["shape"])) for e in f["manifest"]]
