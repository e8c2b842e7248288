"""GPU: dcv_state_pack_multi / _unpack_multi / _digest_multi against runstate.digest_host and the expected bytes, and RunState over whole runs: capture in the
steady state, rollback, exact resume in fresh objects, the optimiser's checkpoint and the fingerprint.  Every comparison is exact."""
import ctypes as C
import struct

import numpy as np
import pytest
import torch

from tests import rig

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
PAD = 8                          # dwords of sentinel on either side of every tensor a kernel reads or writes (32 bytes: the 16-byte grid is kept)
SENTINEL = 0x5A5A5A5A
# dwords, and the source's distance from the 16-byte grid in dwords.  Table 1 (24 tensors) and table 2 (7); one tensor above 24 blocks; an empty one in each table
SIZES = [0, 1, 3, 4, 5, 255, 256, 257, 4095, 4096, 4097, 3 * 4096 + 2, 25 * 4096 + 7, 2, 6, 1023, 1025, 8192, 12, 16, 4094, 4098, 300, 64,
         7, 0, 4099, 2 * 4096, 31, 8, 513]
SHIFTS = [0, 1, 2, 3, 0, 3, 0, 1, 2, 0, 3, 1, 0, 2, 0, 0, 1, 2, 3, 0, 0, 1, 2, 3, 1, 0, 0, 3, 2, 0, 1]


def _bits(v):
    return struct.unpack("<I", struct.pack("<f", float(v)))[0]


def _tab(xs, ctype=C.c_void_p):
    return (ctype * max(len(xs), 1))(*[int(x) for x in xs])


def _contents(gen, k, n):
    """n dwords: fp32 noise, int32, int64 pairs, or fp32 specials (NaN payloads, infinities, -0.0), by the tensor's index."""
    kind = k % 4
    if kind == 0:
        w = gen.standard_normal(n).astype(np.float32).view(np.uint32)
    elif kind == 1:
        w = gen.integers(-2 ** 31, 2 ** 31, size=n).astype(np.int32).view(np.uint32)
    elif kind == 2:
        w = gen.integers(-2 ** 62, 2 ** 62, size=(n + 1) // 2).astype(np.int64).view(np.uint32)[:n]
    else:
        special = np.array([0x7FC00001, 0xFFC12345, 0x7F800000, 0xFF800000, 0x80000000, 0x00000000, 0x7F800001, 0x00000001], dtype=np.uint32)
        w = special[gen.integers(0, len(special), size=n)]
    return np.ascontiguousarray(w, dtype=np.uint32)


def _banded(words, shift):
    """-> (the whole device buffer, the data's address): `words` behind PAD + shift sentinels and in front of PAD more."""
    host = np.full(words.size + 2 * PAD + shift, SENTINEL, dtype=np.uint32)
    host[PAD + shift:PAD + shift + words.size] = words
    buf = torch.from_numpy(host.view(np.int32)).to(DEV)
    assert buf.data_ptr() % 16 == 0
    return buf, buf.data_ptr() + 4 * (PAD + shift), host


# ---- 1. the kernels ---------------------------------------------------------------------------------------------------------------------------------------
def test_pack_unpack_digest_exact():
    from dcvgan_amd import native, runstate as RS
    L, st = native.lib(), native.stream_ptr()
    gen = np.random.default_rng(5)
    n = len(SIZES)
    assert n == len(SHIFTS) > 24 and max(SIZES) > 24 * 4096 and {1, 2, 3} <= set(SHIFTS)
    words = [_contents(gen, k, s) for k, s in enumerate(SIZES)]
    srcs = [_banded(w, sh) for w, sh in zip(words, SHIFTS)]
    assert sorted({(p % 16) for _, p, _ in srcs}) == [0, 4, 8, 12]
    offsets, total = [], 0
    for s in SIZES:
        offsets.append(total)
        total += (s + 3) // 4 * 4
    arena_buf, arena_ptr, arena_host = _banded(np.full(total, 0x77777777, dtype=np.uint32), 0)
    digests = torch.full((n + 2, 2), -7, dtype=torch.int64, device=DEV)
    dwords, offs = _tab(SIZES, C.c_int64), _tab(offsets, C.c_int64)
    need = L.dcv_state_workspace_bytes(n, dwords)
    assert need == sum((s + 4095) // 4096 for s in SIZES) * 16
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    n0 = native.launch_count()
    native.check(L.dcv_state_pack_multi(n, _tab([p for _, p, _ in srcs]), dwords, C.c_void_p(arena_ptr), total, offs, C.c_void_p(digests[1:].data_ptr()),
                                        native.ptr(ws), need, st), "dcv_state_pack_multi")
    assert native.launch_count() - n0 == 4      # two tables: a pack and a fold each
    torch.cuda.synchronize()
    # the arena: the concatenation with zero padding, byte for byte; its bands and the sources untouched
    want = np.zeros(total, dtype=np.uint32)
    for w, o in zip(words, offsets):
        want[o:o + w.size] = w
    got = arena_buf.cpu().numpy().view(np.uint32)
    assert np.array_equal(got[PAD:PAD + total], want)
    assert np.all(got[:PAD] == SENTINEL) and np.all(got[PAD + total:] == SENTINEL)
    for k, (buf, _, host) in enumerate(srcs):
        assert np.array_equal(buf.cpu().numpy().view(np.uint32), host), k
    # the digests: digest_host's, and nothing written outside the table
    dig = digests.cpu().numpy()
    assert np.all(dig[0] == -7) and np.all(dig[-1] == -7)
    want_dig = np.array([RS._signed(RS.digest_host(w)) for w in words], dtype=np.int64)
    assert np.array_equal(dig[1:-1], want_dig)
    assert tuple(dig[1]) == (0, 0) and len({tuple(r) for r in dig[1:-1]}) == n - 1      # the two empty tensors share (0, 0)
    # unpack into fresh sentinel-filled tensors on the same grid offsets: every bit, and the bands
    dsts = [_banded(np.full(s, 0x33333333, dtype=np.uint32), sh) for s, sh in zip(SIZES, SHIFTS)]
    n0 = native.launch_count()
    native.check(L.dcv_state_unpack_multi(n, _tab([p for _, p, _ in dsts]), dwords, C.c_void_p(arena_ptr), total, offs, st), "dcv_state_unpack_multi")
    assert native.launch_count() - n0 == 2
    torch.cuda.synchronize()
    for k, ((buf, _, _), (_, _, host)) in enumerate(zip(dsts, srcs)):
        assert np.array_equal(buf.cpu().numpy().view(np.uint32), host), k
    assert np.array_equal(arena_buf.cpu().numpy().view(np.uint32), got)
    # the digests alone: of the arena's segments (all on the 16-byte grid) and of the live sources (some off it) — the pack's
    for ptrs in ([arena_ptr + 4 * o for o in offsets], [p for _, p, _ in srcs]):
        again = torch.full((n + 2, 2), -7, dtype=torch.int64, device=DEV)
        n0 = native.launch_count()
        native.check(L.dcv_state_digest_multi(n, _tab(ptrs), dwords, C.c_void_p(again[1:].data_ptr()), native.ptr(ws), need, st), "dcv_state_digest_multi")
        assert native.launch_count() - n0 == 4
        torch.cuda.synchronize()
        assert np.array_equal(again.cpu().numpy(), dig)
    assert np.array_equal(arena_buf.cpu().numpy().view(np.uint32), got)      # a digest copies nothing
    # a table without dwords: only the fold runs and writes (0, 0)
    empty = torch.full((3, 2), -7, dtype=torch.int64, device=DEV)
    n0 = native.launch_count()
    native.check(L.dcv_state_digest_multi(1, _tab([0]), _tab([0], C.c_int64), C.c_void_p(empty[1:].data_ptr()), native.ptr(ws), need, st), "dcv_state_digest_multi")
    assert native.launch_count() - n0 == 1
    assert empty.cpu().tolist() == [[-7, -7], [0, 0], [-7, -7]]


# ---- whole runs -------------------------------------------------------------------------------------------------------------------------------------------
def _videos(gen, cfg, count=5, frames=20):
    geo = (lambda: gen.integers(0, 256, size=(frames, 64, 64, 1), dtype=np.uint8)) if cfg.geometric_info == "depth" else \
        (lambda: (gen.standard_normal((frames, 64, 64, 2)) * 9).astype(np.float32))
    return [(gen.integers(0, 256, size=(frames, 64, 64, 3), dtype=np.uint8), geo()) for _ in range(count)]


def _build(seed, options, name="isogd-depth"):
    """A run on the device.  `options`: guard (max_norm, dynamic), EMA, spectral normalisation, adaptive augmentation (interval 1), LeCam (start 0) and a
    ClipSampler over five 20-frame videos; without them fixed batches.  t_rand comes from a random stream of the caller's (`free`, no fixed seed: it follows
    torch's) and a count kept in `extra`."""
    from dcvgan_amd import clipstore, native, trainer
    from dcvgan_amd.rng import PhiloxRng
    native.lib()
    cfg = rig.small_cfg(name)
    models, _ = rig.seeded_models(cfg, DEV, seed, seed + 50)
    opts = trainer.build_optimizers(cfg, models, guard=dict(max_norm=10.0, dynamic=True, loss_scale=4.0, growth_interval=2) if options else None)
    sn = ema = aug = lc = sampler = data = None
    if options:
        sn = trainer.build_spectral_norm(cfg, models, opts, seed=seed)
        ema = trainer.build_ema(cfg, models, opts)
        aug = trainer.build_augment(cfg, models, opts, p=0.5, interval=1, adjust_clips=8, seed=seed + 3)
        lc = trainer.build_lecam(cfg, models, opts, weight=0.3, start=0, one_sided=False)
        store = clipstore.ClipStore.from_arrays(_videos(np.random.default_rng(77), cfg), cfg.video_length, cfg.geometric_info, DEV)
        sampler = trainer.build_clip_sampler(cfg, store, seed=seed + 9, rank=0, world=1)
    else:
        data = rig.clip_pair(cfg, DEV, 4)
    runner = trainer.StepRunner(cfg, models, opts, trainer.build_loss(cfg), ema=ema, spectral=sn, augment=aug, lecam=lc)
    free, extra = PhiloxRng(), {"t_count": 0, "seed": seed}
    rs = trainer.build_run_state(cfg, models, opts, runner=runner, ema=ema, spectral=sn, augment=aug, lecam=lc, sampler=sampler, rngs=(free,), extra=extra)
    return dict(cfg=cfg, models=models, opts=opts, runner=runner, rs=rs, sampler=sampler, data=data, free=free, extra=extra, ema=ema, aug=aug, lc=lc, sn=sn)


def _iterate(run, n, fingerprints=None):
    """n iterations -> their outputs as bits.  `fingerprints`: a list that receives fingerprint_host() after each."""
    outs = []
    for _ in range(n):
        seed, off = run["free"]._next()
        run["extra"]["t_count"] += 1
        t = (seed + 5 * off + run["extra"]["t_count"]) % run["cfg"].video_length
        if run["sampler"] is not None:
            batch = run["sampler"].next_batch()
            xc, xg = batch["color"], batch[run["cfg"].geometric_info]
        else:
            xc, xg = run["data"]
        out = run["runner"].step(xc, xg, t)
        outs.append(dict(out, t=t))
        if fingerprints is not None:
            fingerprints.append(run["rs"].fingerprint_host())
    torch.cuda.synchronize()
    return [{k: (v if k == "t" else _bits(v)) for k, v in o.items()} for o in outs]


def _all_bytes(run):
    torch.cuda.synchronize()
    lay = run["rs"]._layout()
    return {n: rig.byte_view(t).clone() for n, t in zip(lay.names, lay.tensors)}


def _host_state(run):
    """The host scalars, with a random stream named by the seed it draws from (a pinned stream and one that follows torch's seed are the same stream)."""
    h = run["rs"]._host_scalars()
    h["rngs"] = [(r["seed_seen"], r["counter"]) for r in h["rngs"][1:]]      # (the process-wide stream is every run's: nothing here draws from it)
    return h


def test_capture_in_the_steady_state():
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    from dcvgan_amd import native
    run = _build(31, True)
    rs = run["rs"]
    _iterate(run, 1)
    first = rs.capture()      # arenas, digest tables, workspace and argument arrays are made here
    rs.fingerprint()          # (and the fingerprint's table)
    torch.cuda.synchronize()
    per = rs.launches_per_capture()
    n_entries = len(rs.manifest())
    assert per == 2 * ((n_entries + 23) // 24) and n_entries > 200
    m0 = torch.cuda.memory_allocated()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        torch.cuda.set_sync_debug_mode("error")      # (inside the profiler's own start / stop, which synchronise)
        try:
            n0 = native.launch_count()
            second = rs.capture()
            n1 = native.launch_count()
            third = rs.capture()
            n2 = native.launch_count()
            fp = rs.fingerprint()
            n3 = native.launch_count()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        m1 = torch.cuda.memory_allocated()
        torch.cuda.synchronize()
    assert n1 - n0 == per and n2 - n1 == per and n3 - n2 == per
    kernels = {e.key: e.count for e in prof.key_averages() if e.device_type == DeviceType.CUDA}
    foreign = {k[:160]: c for k, c in kernels.items() if "at::" in k or "torch" in k.lower()}
    assert not foreign, foreign
    assert sum(kernels.values()) == 3 * per and all("rs_kernel" in k or "rs_final_kernel" in k for k in kernels), kernels
    assert m1 == m0      # nothing is allocated after the first call
    assert third.arena is first.arena and second.arena is not first.arena      # a ring of two
    # the three captures hold the same bytes and the live state's digests
    assert torch.equal(second.arena, third.arena) and torch.equal(second.digests, third.digests) and torch.equal(fp, third.digests)
    assert fp.is_cuda and fp.dtype == torch.int64 and tuple(fp.shape) == (n_entries, 2)
    print(f"\n[runstate capture] {n_entries} entries, {rs.arena_bytes()} bytes, {per} launches per capture")


def test_rollback():
    from dcvgan_amd import runstate as RS
    run = _build(32, True)
    rs = run["rs"]
    _iterate(run, 2)
    snap = rs.capture()
    fps = []
    want = _iterate(run, 2, fps)
    assert run["runner"].iteration == 4 and RS.RunState.diff(fps[0], fps[1])
    snap.restore()
    assert run["runner"].iteration == 2 and run["extra"]["t_count"] == 2
    again = []
    got = _iterate(run, 2, again)
    assert got == want and len(want[0]) > 8
    assert [RS.RunState.diff(a, b) for a, b in zip(fps, again)] == [[], []]


@pytest.mark.parametrize("options,name", [(True, "isogd-depth"), (False, "isogd-flow")])
def test_resume_in_fresh_objects(options, name, tmp_path):
    """Run A: four iterations.  Run B: two, save, discard; everything rebuilt from other seeds, load + restore, two more.  Iterations 3 and 4 agree in every loss
    bit, and afterwards in every state tensor and host scalar.  The same rebuilt objects without the load give other losses."""
    from dcvgan_amd import runstate as RS
    a = _build(40, options, name)
    fp_a = []
    out_a = _iterate(a, 4, fp_a)
    bytes_a, host_a = _all_bytes(a), _host_state(a)
    b = _build(40, options, name)
    out_b = _iterate(b, 2)
    assert out_b == out_a[:2]      # (the premise: two seeded runs are the same run)
    path = str(tmp_path / "run.pt")
    b["rs"].capture().save(path)
    del b
    c = _build(41, options, name)
    c["free"]._next()      # the fresh objects have lived a little: another seed, other counters
    c["rs"].load(path).restore()
    assert c["free"]._fixed_seed == 40 and torch.initial_seed() == 41      # pinned to the stream it was; torch's seed is not touched
    fp_c = []
    out_c = _iterate(c, 2, fp_c)
    first = [RS.RunState.diff(x, y) for x, y in zip(fp_a[2:], fp_c)]
    assert first == [[], []], f"diverged first in {first[0][:5] or first[1][:5]}"
    assert out_c == out_a[2:]
    bytes_c = _all_bytes(c)
    assert bytes_c.keys() == bytes_a.keys() and len(bytes_a) > 100
    assert [k for k in bytes_a if not torch.equal(bytes_a[k], bytes_c[k])] == []
    assert _host_state(c) == host_a
    assert c["runner"].iteration == 4 and c["extra"] == a["extra"] == {"t_count": 4, "seed": 40}
    if options:
        assert (c["sampler"].epoch, c["sampler"].iteration) == (a["sampler"].epoch, a["sampler"].iteration) == (2, 0)
        assert c["ema"].num_updates() == a["ema"].num_updates() > 0 and c["aug"].state_words() == a["aug"].state_words()
    # the generators a sampler would load, cut out of the file: run B's after two iterations
    sd = RS.model_state_dict(path, "ggen")
    assert list(sd) == list(a["models"]["ggen"].state_dict()) and all(not v.is_cuda for v in sd.values())
    # control: the same rebuilt objects WITHOUT the load
    d = _build(41, options, name)
    d["free"]._next()
    out_d = _iterate(d, 2)
    assert all(out_d[i][k] != out_a[2 + i][k] for i in range(2) for k in ("loss_gen", "loss_idis", "loss_vdis", "loss_gdis"))


# ---- 5. the optimiser's checkpoint ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("guarded", [False, True])
def test_adam_state_dict_round_trip_on_the_device(guarded):
    from dcvgan_amd import native, optim
    native.lib()
    gen = torch.Generator().manual_seed(8)
    shapes = [(5000,), (17,), (4, 1024), (3, 3)]
    init = [torch.randn(s, generator=gen) for s in shapes]
    grads = [[torch.randn(s, generator=gen) for s in shapes] for _ in range(3)]

    def make():
        ps = [torch.nn.Parameter(t.clone().to(DEV)) for t in init]
        g = optim.GradGuard(max_norm=1.0, dynamic=True, loss_scale=2.0, growth_interval=2) if guarded else None
        return ps, optim.Adam(ps, lr=1e-2, betas=(0.5, 0.999), weight_decay=1e-5, guard=g), g

    def step(ps, o, g, k):
        for p, gr in zip(ps[:3], grads[k]):      # the last parameter gets no gradient: no state
            p.grad = gr.to(DEV)
        if g is not None:
            g.measure()
        o.step()

    ps1, o1, g1 = make()
    step(ps1, o1, g1, 0); step(ps1, o1, g1, 1)
    sd = o1.state_dict()
    assert sorted(sd["state"]) == [0, 1, 2] and all(float(sd["state"][i]["step"]) == 2.0 and sd["state"][i]["exp_avg"].is_cuda for i in sd["state"])
    ps2, o2, g2 = make()
    with torch.no_grad():
        for p, q in zip(ps2, ps1):
            p.copy_(q)
    o2.load_state_dict(sd)
    if guarded:
        g2.load_state_dict(g1.state_dict())
        assert g2.measurements == 2 and torch.equal(g2.state, g1.state)
        assert len({o2.state[p]["step_block"].data_ptr() for p in ps2[:3]}) == 1
    # torch's own Adam takes the same dict
    torch.optim.Adam(ps2, lr=1.0).load_state_dict(o1.state_dict())
    step(ps1, o1, g1, 2); step(ps2, o2, g2, 2)
    torch.cuda.synchronize()
    for p, q in zip(ps1, ps2):
        assert torch.equal(p.detach().view(torch.int32), q.detach().view(torch.int32))
    s1, s2 = o1.state_dict(), o2.state_dict()
    for i in (0, 1, 2):
        assert float(s1["state"][i]["step"]) == float(s2["state"][i]["step"]) == 3.0
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(s1["state"][i][k].view(torch.int32), s2["state"][i][k].view(torch.int32))
    assert not torch.equal(ps1[0].detach().cpu(), init[0])
    if guarded:
        assert torch.equal(g1.state, g2.state)


# ---- 6. the fingerprint -----------------------------------------------------------------------------------------------------------------------------------
def test_fingerprint_tells_one_ulp():
    from dcvgan_amd import runstate as RS
    a, b = _build(50, False), _build(50, False)
    _iterate(a, 1); _iterate(b, 1)
    fa, fb = a["rs"].fingerprint_host(), b["rs"].fingerprint_host()
    assert RS.RunState.diff(fa, fb) == [] and len(fa) > 100
    lay = a["rs"]._layout()
    for n, t in list(zip(lay.names, lay.tensors))[::7]:      # a sample of entries against the host mirror
        assert fa[n] == tuple(RS._signed(RS.digest_host(t))), n
    key = list(b["models"]["vdis"].state_dict())[0]
    w = b["models"]["vdis"].state_dict(keep_vars=True)[key]
    with torch.no_grad():
        w.view(-1).view(torch.int32)[3] += 1      # one ulp
    assert RS.RunState.diff(fa, b["rs"].fingerprint_host()) == [f"model.vdis.{key}"]
    assert RS.RunState.diff(b["rs"].fingerprint_host(), fa) == [f"model.vdis.{key}"]
