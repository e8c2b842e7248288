"""GPU: the autograd plumbing of dcvgan_amd/ops.py against its fp64 host twin (tests/exactgraph.py), word for word.

Every case builds a small graph through ops.* with outputs and gradients pre-filled with NaN (ops._POISON), runs one call pattern, and compares the forward values,
every input gradient and every parameter gradient with the twin's — the operands are integers, so the twin's values ARE the fp32 words (proved on the host,
tests/test_graph_exact_cpu.py).  A recording proxy over the library handle notes every entry point: each case asserts the multiset of launches it expects, so a route
that quietly falls back fails instead of passing on the fallback's correct result.  Every route is also switched off through its module attribute and compared with
itself switched on, bit for bit.  Nothing here provokes the device: the one exception raised on purpose (pattern `hook_raises`) is a Python exception on the host."""
import functools
import itertools
from collections import Counter, OrderedDict

import pytest
import torch

from tests import exactbn as XB
from tests import exactgraph as G

pytestmark = pytest.mark.gpu
SWITCHES = ("_SKIP_ACCUMULATE", "_GATED_DGRAD", "_OWN_ACCUMULATION", "_WGRAD_SIDE", "_USE_PACK_CACHE")      # (_HEAD_BN_FUSION: test_bn_link_refused_or_empty, the only graphs with a link)
WORDS = [0]


@pytest.fixture(scope="module")
def dev():
    from dcvgan_amd import native
    native.lib()
    return torch.device("cuda:0")


@pytest.fixture
def rec(monkeypatch, dev):
    """NaN-filled outputs and the recording proxy, both undone by monkeypatch when the test ends"""
    from dcvgan_amd import native, ops, ops_cl
    monkeypatch.setattr(ops, "_POISON", True)
    r = G.Recorder(native.lib())
    monkeypatch.setattr(ops, "lib", r)
    monkeypatch.setattr(ops_cl, "lib", r)
    yield r
    torch.cuda.synchronize()


@functools.lru_cache(maxsize=None)
def twin(name, pattern, frozen=None):
    """The host's results, computed and proved once per (graph, pattern) and shared"""
    return G.prove(G.GRAPHS[name], pattern, frozen if frozen is not None else G.FROZEN.get(pattern, ()))[0]


def compare(what, got, want):
    assert list(got) == list(want), (what, list(got), list(want))
    bad = [m for m in (G.mismatch(f"{what} {n}", got[n], want[n]) for n in want) if m]
    assert not bad, "\n".join(bad)
    WORDS[0] += sum(t.numel() for t in want.values() if t is not None)


def same(what, a, b):
    assert list(a) == list(b)
    bad = [n for n in a if not G.same_words(a[n], b[n])]
    assert not bad, f"{what}: not bit-identical: {bad}"
    WORDS[0] += sum(t.numel() for t in a.values() if t is not None)


def fmt(marks):
    return [(l, dict(sorted(c.items()))) for l, c in marks]


# ------------------------------------------------------------------------------------------------------------------------------------------------------
# graphs x call patterns against the twin
# ------------------------------------------------------------------------------------------------------------------------------------------------------
CASES = [(n, p) for n in G.GRAPHS for p in (G.PATTERNS if n in G.PATTERN_GRAPHS else ("once",))]


@pytest.mark.parametrize("name,pattern", CASES, ids=[f"{n}-{p}" for n, p in CASES])
def test_graph_against_twin(dev, rec, name, pattern):
    graph = G.GRAPHS[name]
    got, marks = G.run_pattern(G.Device(dev), graph, pattern, rec, G.FROZEN.get(pattern, ()))
    print(f"graph-exact {name} {pattern}: {fmt(marks)}")
    compare(f"{name} {pattern}", got, twin(name, pattern))
    want = G.expected_marks(graph, pattern)
    if want is not None:
        assert fmt(marks) == fmt(want), f"launches differ from the case table:\n got      {fmt(marks)}\n expected {fmt(want)}"
    total = sum((c for _, c in marks), Counter())
    if pattern in ("no_weight", "neither"):      # a frozen weight: no weight-gradient entry of any kind ran
        assert not [k for k in total if "backward_weight" in k], total
    if pattern in ("no_input", "neither"):       # no data gradient for a leaf input: only the inner convolutions' data gradients are left
        inner = {"unet_s0.25": 3, "dfront_s0.25": 1, "psum_s0.25": 0}[name] if pattern == "no_input" else 0
        assert sum(v for k, v in total.items() if "backward_data" in k) == inner, total
    if pattern == "neither":
        assert sum(total.values()) == sum(graph.fwd.values()), total
    if pattern == "grad_beside_grads":           # .grad is what the first backward left, word for word
        for n, t in got.items():
            if n.startswith("kept"):
                assert G.same_words(t, got["before:" + n.split(":")[1]]), n
    if pattern == "retain_twice":                # integers: the second backward doubles every gradient exactly
        for n, t in got.items():
            if n.startswith("second:"):
                assert torch.equal(t, 2 * got["first:" + n[7:]]), n


@pytest.mark.parametrize("name", list(G.GRAPHS))
def test_layers_run_adds_nothing(dev, rec, name):
    """Every graph with its convolutions as torch modules under dcvgan_amd.layers.run (which holds no library handle of its own: it calls ops.*): the same launches
    mark by mark and the same words as the direct ops build, and the twin's words"""
    graph = G.GRAPHS[name]
    for pattern in (("once", "retain_twice", "two_forwards_summed") if name in G.PATTERN_GRAPHS else ("once",)):
        direct, marks_d = G.run_pattern(G.Device(dev), graph, pattern, rec)
        via, marks_l = G.run_pattern(G.DeviceLayers(dev), graph, pattern, rec)
        assert fmt(marks_l) == fmt(marks_d) == fmt(G.expected_marks(graph, pattern))
        same(f"{name} {pattern} layers.run", via, direct)
        compare(f"{name} {pattern} layers.run", via, twin(name, pattern))


@pytest.mark.parametrize("name", ["dfront_s0.25", "dfront_s0.0", "dfront3d_s0.25"])
@pytest.mark.parametrize("frozen", [(), ("xc",), ("xg",), ("wg", "wc"), ("xc", "wc")], ids=["all", "xc_frozen", "xg_frozen", "stem_weights_frozen", "one_stem_dead"])
def test_stem_gate_count(dev, rec, name, frozen):
    """The gated data gradient of the trunk sets act_applied = 2 and each stem that runs takes one off; neither stem calls dcv_act_backward"""
    graph = G.GRAPHS[name]
    B = G.Device(dev)
    L = graph.leaves(B, frozen)
    outs, taps = graph.fn(B, L)
    slot, seen = taps["buf"].slot, []
    assert slot.act_applied is False
    for k in ("first", "skip"):
        if taps[k].requires_grad:
            taps[k].register_hook(lambda g, k=k: seen.append((k, int(slot.act_applied))))
    rec.reset()
    torch.autograd.backward(outs, graph.cotangents(B))
    c = rec.launches()
    stems = sum(1 for k in ("first", "skip") if taps[k].requires_grad)
    assert [v for _, v in seen] == [2, 1][:stems], seen
    assert int(slot.act_applied) == 2 - stems
    assert c["dcv_conv_backward_data_gated"] == 1 and c["dcv_act_backward"] == 0 and not [k for k in c if k.endswith("!refused")], c
    got = OrderedDict(y=B.value(outs[0]))
    G._grads(B, L, got, "")
    compare(f"{name} frozen {frozen}", got, twin(name, "once", tuple(frozen)))


def test_unet_slot_state(dev, rec):
    """The conv node of the skip's consumer returns no dx of its own (the slot's slice took it), the slot is empty afterwards and act_applied is back to 0"""
    graph = G.GRAPHS["unet_s0.25"]
    B = G.Device(dev)
    L = graph.leaves(B)
    outs, taps = graph.fn(B, L)
    slot, seen = taps["buf"].slot, []
    taps["skip"].register_hook(lambda g: seen.append((slot.g is None, bool(slot.act_applied), g.data_ptr(), tuple(g.stride()))))
    torch.autograd.backward(outs, graph.cotangents(B), retain_graph=True)
    # at the producer: the slot was taken, the derivative is marked applied, and the gradient it receives is the join's slice itself (a strided view: nothing was added
    # by autograd, which would have produced a dense tensor)
    assert len(seen) == 1 and seen[0][0] and seen[0][1] and seen[0][3][0] == 16 * 64, seen
    assert slot.g is None and int(slot.act_applied) == 0


@pytest.mark.parametrize("augmented", [False, True], ids=["fan_out", "fan_geometry"])
def test_segmentation_front(dev, rec, monkeypatch, augmented):
    """The generators' front as the segmentation iteration has it (G.segmfront_graph): the clip's four readers, of which the colour generator — segm_onehot under
    no_grad into a stem whose act_slot is armed — hands back None.  The clip's gradient and all seven weight gradients are the twin's words; the stem has a weight
    gradient and NO data-gradient entry (six for seven convolutions), its derivative pass is the consumer's gated epilogue, and the slot is left empty.  With
    augment.fan_geometry (p = 1, a fixed table of flips, shifts and cutouts) in fan_out's place: _AugFan's missing-gradient branch, one dcv_aug_fan_backward."""
    from dcvgan_amd import augment
    monkeypatch.setattr(augment, "lib", rec)
    graph = G.segmfront_graph(0.25, augmented)
    B = G.Device(dev)
    L = graph.leaves(B)
    rec.reset()
    outs, taps = graph.fn(B, L)
    fwd = rec.launches()
    assert not taps["maps"].requires_grad and taps["buf"].slot.act is not None and taps["buf"].slot.act_applied is False
    seen = []
    taps["skip"].register_hook(lambda g: seen.append((taps["buf"].slot.g is None, int(taps["buf"].slot.act_applied))))
    rec.reset()
    torch.autograd.backward(outs, graph.cotangents(B))
    bwd = rec.launches()
    print(f"graph-exact {graph.name}: fwd {dict(sorted(fwd.items()))} bwd {dict(sorted(bwd.items()))}")
    got = OrderedDict(y=B.value(outs[0]))
    G._grads(B, L, got, "")
    want = G.prove(graph, "once")[0]
    compare(graph.name, got, want)
    assert got["dx"] is not None and bool((got["dx"] != 0).any())
    assert fwd == graph.fwd and bwd == graph.bwd, (fwd, bwd)
    assert sum(v for k, v in bwd.items() if "backward_data" in k) == 6 and sum(v for k, v in bwd.items() if "backward_weight" in k) == 7 and not [k for k in bwd if "!" in k]
    assert seen == [(True, 1)] and taps["buf"].slot.g is None and int(taps["buf"].slot.act_applied) == 0


# ------------------------------------------------------------------------------------------------------------------------------------------------------
# every route ON against OFF, bit for bit
# ------------------------------------------------------------------------------------------------------------------------------------------------------
ONOFF_PATTERNS = ("once", "retain_twice", "pruned_first", "grad_beside_grads", "two_forwards_summed", "two_forwards_sequential", "cot_expand", "cot_broadcast")


@pytest.mark.parametrize("switch", SWITCHES)
@pytest.mark.parametrize("name", list(G.GRAPHS))
def test_route_on_equals_off(dev, rec, monkeypatch, name, switch):
    from dcvgan_amd import ops
    graph = G.GRAPHS[name]
    for pattern in (ONOFF_PATTERNS if name in G.PATTERN_GRAPHS else ("once",)):
        assert getattr(ops, switch) is True
        on, marks_on = G.run_pattern(G.Device(dev), graph, pattern, rec)
        with monkeypatch.context() as m:
            m.setattr(ops, switch, False)
            off, marks_off = G.run_pattern(G.Device(dev), graph, pattern, rec)
        same(f"{name} {pattern} {switch}", on, off)
        compare(f"{name} {pattern} {switch} off", off, twin(name, pattern))
        tot_on, tot_off = sum((c for _, c in marks_on), Counter()), sum((c for _, c in marks_off), Counter())
        gated = tot_on["dcv_conv_backward_data_gated"]
        if switch == "_GATED_DGRAD" or (switch == "_SKIP_ACCUMULATE" and name.startswith(("unet", "segmfront"))):
            # the two-step route: no gated call at all (not even a refused one), the derivative passes come back
            assert not [k for k in tot_off if "gated" in k], tot_off
            stems = 2 if name.startswith("dfront") else 1
            if pattern != "pruned_first":      # (there the pruned pass runs the gated consumer without its producers)
                assert tot_off["dcv_act_backward"] == tot_on["dcv_act_backward"] + gated * stems, (tot_on, tot_off)
        elif switch == "_SKIP_ACCUMULATE" and name.startswith("dfront"):
            assert not [k for k in tot_off if "gated" in k], tot_off       # no slot, no gate
        elif switch == "_OWN_ACCUMULATION":
            assert tot_off["dcv_conv_backward_weight_acc"] == 0 and \
                tot_off["dcv_conv_backward_weight"] == tot_on["dcv_conv_backward_weight"] + tot_on["dcv_conv_backward_weight_acc"], (tot_on, tot_off)
        else:
            assert tot_on == tot_off, (switch, tot_on, tot_off)


def test_companion_stream_is_taken(dev, rec):
    """_WGRAD_SIDE on: the weight gradients of a default-stream backward are launched on the companion stream (and joined: the results above are read after it)"""
    from dcvgan_amd import ops
    graph = G.GRAPHS["psum_s0.25"]
    B = G.Device(dev)
    L = graph.leaves(B)
    outs, _ = graph.fn(B, L)
    streams = []
    real = rec._real.dcv_conv_backward_weight

    class Spy:
        def __getattr__(self, n):
            return getattr(keep, n)

        def dcv_conv_backward_weight(self, *a):
            streams.append(torch.cuda.current_stream().cuda_stream)
            return real(*a)
    keep = rec._real
    rec._real = Spy()
    try:
        torch.autograd.backward(outs, graph.cotangents(B))
    finally:
        rec._real = keep
    assert len(streams) == 1 and streams[0] != torch.cuda.default_stream().cuda_stream
    assert ops._side_streams and streams[0] == ops._side_streams[dev.index].cuda_stream


# ------------------------------------------------------------------------------------------------------------------------------------------------------
# parameter sums: an existing .grad, a .grad the in-place sum must refuse; BatchNorm and GRU parameters through deliver_small
# ------------------------------------------------------------------------------------------------------------------------------------------------------
def _psum_conv(dev, rec, prior):
    """The psum graph on two batches in one backward, with `prior`: None, "dense" (a contiguous .grad) or "strided" (one the in-place sum refuses)"""
    graph = G.GRAPHS["psum_s0.25"]
    out = []
    for B in (G.Device(dev), G.Host()):
        L = graph.leaves(B)
        L2 = graph.leaves(B, tag=":fake", share=L)
        g = torch.Generator().manual_seed(G.seed_of("psum-prior"))
        g0 = G.ints(g, (8, 8, 4, 8))
        if prior == "dense":
            L["w"].grad = B.cot(g0)[..., ::2].contiguous()
        elif prior == "strided":
            L["w"].grad = B.cot(g0)[..., ::2]
            assert not L["w"].grad.is_contiguous()
        if rec is not None and isinstance(B, G.Device):
            rec.reset()
        ya, _ = graph.fn(B, L)
        yb, _ = graph.fn(B, L2)
        ca, cb = graph.cotangents(B), graph.cotangents(B, ":fake")
        torch.autograd.backward(ya + yb, ca + cb)
        out.append(OrderedDict(dw=B.value(L["w"].grad), dx=B.value(L["x"].grad), dx2=B.value(L2["x"].grad)))
    assert all(G.is_f32(t) for t in out[1].values())
    return out


@pytest.mark.parametrize("prior", [None, "dense", "strided"], ids=["no_grad_yet", "grad_present", "grad_refused"])
def test_conv_parameter_sum(dev, rec, monkeypatch, prior):
    from dcvgan_amd import ops
    got, want = _psum_conv(dev, rec, prior)
    c = rec.launches()
    compare(f"psum conv {prior}", got, want)
    # first contribution by the plain entry, later ones by the accumulating one; a refused .grad leaves both to autograd's add
    assert (c["dcv_conv_backward_weight"], c["dcv_conv_backward_weight_acc"]) == {None: (1, 1), "dense": (0, 2), "strided": (2, 0)}[prior], c
    for switch in ("_OWN_ACCUMULATION", "_WGRAD_SIDE"):
        with monkeypatch.context() as m:
            m.setattr(ops, switch, False)
            off, _ = _psum_conv(dev, rec, prior)
        same(f"psum conv {prior} {switch}", got, off)


def _bn_operands(tag):
    o = XB.exact_operands("graph-psum-bn" + tag, (2, 8, 8, 8))
    return o


def _psum_bn(dev, prior):
    """One BatchNorm + LeakyReLU(1/4) group on two batches (tests/exactbn.py's integer scheme: dgamma and dbeta are exact) -> device results, fp64 expectations"""
    from dcvgan_amd import ops
    o1, o2 = _bn_operands(":a"), _bn_operands(":b")
    o2 = o2._replace(gamma=o1.gamma, beta=o1.beta)
    refs = [XB.reference(o, "leaky", eps=0.0) for o in (o1, o2)]
    for o, r in zip((o1, o2), refs):
        assert XB.sums_exact(o, r, XB.RUN32, "leaky") and XB.stats_exact(o, r)
    g0 = G.ints(torch.Generator().manual_seed(5), (2, 8, 2))
    prior_g = {None: None, "dense": g0[..., 0].contiguous(), "strided": g0[..., 0]}[prior]
    gamma, beta = torch.nn.Parameter(o1.gamma.float().to(dev)), torch.nn.Parameter(o1.beta.float().to(dev))
    if prior_g is not None:
        pg = prior_g.float().to(dev) if prior == "dense" else g0.float().to(dev)[..., 0]
        gamma.grad, beta.grad = pg[0], pg[1]
        assert gamma.grad.is_contiguous() == (prior == "dense")
    xs = [o.x.float().to(dev).requires_grad_(True) for o in (o1, o2)]
    ys = [ops.bn_act(x, gamma, beta, None, None, True, ops.ACT_LEAKY, XB.SLOPE, eps=0.0) for x in xs]
    torch.autograd.backward(ys, [o.dy.float().to(dev) for o in (o1, o2)])
    base = (prior_g[0], prior_g[1]) if prior_g is not None else (0.0, 0.0)
    want = OrderedDict(dgamma=refs[0].dgamma + refs[1].dgamma + base[0], dbeta=refs[0].dbeta + refs[1].dbeta + base[1])
    assert all(G.is_f32(t) for t in want.values())
    got = OrderedDict(dgamma=gamma.grad.detach().cpu(), dbeta=beta.grad.detach().cpu())
    return got, want


@pytest.mark.parametrize("prior", [None, "dense", "strided"], ids=["no_grad_yet", "grad_present", "grad_refused"])
def test_bn_parameter_sum(dev, rec, monkeypatch, prior):
    from dcvgan_amd import ops
    rec.reset()
    got, want = _psum_bn(dev, prior)
    c = rec.launches()
    compare(f"psum bn {prior}", got, want)
    # deliver_small adds the later contributions of gamma and of beta with one dcv_axpby each
    assert c["dcv_bn_act_backward"] == 2 and c["dcv_axpby"] == {None: 2, "dense": 4, "strided": 0}[prior], c
    for switch in ("_OWN_ACCUMULATION", "_WGRAD_SIDE"):
        with monkeypatch.context() as m:
            m.setattr(ops, switch, False)
            off, _ = _psum_bn(dev, prior)
        same(f"psum bn {prior} {switch}", got, off)


def _gru_operands(tag):
    from tests import exactew as XE
    return XE.gru_operands(3, 2, 4)


def _psum_gru(dev, prior, uses=(0, 1)):
    """The GRU of (T, B, dm) = (3, 2, 4) on one or two input sets (the second: the first's operands reversed along their first axis; same parameters)"""
    from dcvgan_amd import ops
    oa = _gru_operands("")
    ob = dict(oa, e=oa["e"].flip(0), h0=oa["h0"].flip(0), dout=oa["dout"].flip(1))
    names = ("w_ih", "w_hh", "b_ih", "b_hh")
    P = [torch.nn.Parameter(oa[n].float().to(dev)) for n in names]
    g = torch.Generator().manual_seed(11)
    priors = [torch.randn(tuple(p.shape) + (2,), generator=g).to(dev) for p in P]
    if prior is not None:
        for p, q in zip(P, priors):
            p.grad = q[..., 0].contiguous() if prior == "dense" else q[..., 0]
    before = [q[..., 0].cpu().clone() for q in priors]      # (a strided .grad aliases `priors`: autograd adds into it in place)
    outs, cots = [], []
    for i, o in enumerate((oa, ob)):
        if i in uses:
            outs.append(ops.gru_sequence(o["e"].float().to(dev), o["h0"].float().to(dev), *P))
            cots.append(o["dout"].float().to(dev))
    torch.autograd.backward(outs, cots)
    return OrderedDict((n, p.grad.detach().cpu().contiguous()) for n, p in zip(names, P)), before


@pytest.mark.parametrize("prior", [None, "dense", "strided"], ids=["no_grad_yet", "grad_present", "grad_refused"])
def test_gru_parameter_sum(dev, rec, monkeypatch, prior):
    """The GRU's gradients are not integers: the sum is checked against its own parts — each use's gradient taken alone, then added in fp32 on the host in the order
    the backward adds them (.grad, then the later use's node first: it was recorded last) — bit for bit, and against the fp64 recurrence at exactew's bar."""
    from dcvgan_amd import ops
    from tests import exactew as XE
    rec.reset()
    got, priors = _psum_gru(dev, prior)
    c = rec.launches()
    assert c["dcv_gru_backward"] == 2 and c["dcv_axpby"] == {None: 4, "dense": 8, "strided": 0}[prior], c
    (ga, _), (gb, _) = _psum_gru(dev, None, (0,)), _psum_gru(dev, None, (1,))
    for (n, t), q in zip(got.items(), priors):
        want = gb[n] + ga[n] if prior is None else (q + gb[n]) + ga[n] if prior == "dense" else q + (gb[n] + ga[n])
        assert G.same_words(t, want), f"{n}: the sum is not the fp32 sum of its parts"
    WORDS[0] += sum(t.numel() for t in got.values())
    H = G.Host()
    oa = _gru_operands("")
    ob = dict(oa, e=oa["e"].flip(0), h0=oa["h0"].flip(0), dout=oa["dout"].flip(1))
    Pm = [oa[n].clone().requires_grad_(True) for n in ("w_ih", "w_hh", "b_ih", "b_hh")]
    torch.autograd.backward([H.gru(o["e"], o["h0"], *Pm) for o in (oa, ob)], [o["dout"] for o in (oa, ob)])
    for (n, t), p, q in zip(got.items(), Pm, priors):
        ref = p.grad + (q.double() if prior is not None else 0.0)
        print(f"graph-exact gru {prior} {n}: rel_l2 {XE.rel_l2(t, ref):.3g}")
        assert XE.rel_l2(t, ref) < 5 * 2e-7, (n, XE.rel_l2(t, ref))
    for switch in ("_OWN_ACCUMULATION", "_WGRAD_SIDE"):
        with monkeypatch.context() as m:
            m.setattr(ops, switch, False)
            off, _ = _psum_gru(dev, prior)
        if switch == "_OWN_ACCUMULATION" and prior == "dense":
            # two uses in one backward BESIDE an existing .grad: the in-place route adds (grad + g2) + g1, autograd grad + (g2 + g1) — the same three operands in
            # another association.  Exactly summable gradients (the convolution and BatchNorm cases above) are bit-identical; these are not integers, so each
            # side is held to its own association, bit for bit (the training iteration has no such pass)
            for (n, t), q in zip(off.items(), priors):
                assert G.same_words(t, q + (gb[n] + ga[n])), f"{n}: autograd's sum is not grad + (g2 + g1)"
            differ = sum(int((off[n] != got[n]).sum()) for n in got)
            print(f"graph-exact gru dense: {differ} of {sum(t.numel() for t in got.values())} words differ between the two associations")
            continue
        same(f"psum gru {prior} {switch}", got, off)


# ------------------------------------------------------------------------------------------------------------------------------------------------------
# fan_out, temporal_diff, cat_channels / copy_into, loss sums
# ------------------------------------------------------------------------------------------------------------------------------------------------------
class _Drop(torch.autograd.Function):
    """A consumer that delivers no gradient"""

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return None


def _fan_x(B, layout):
    g = torch.Generator().manual_seed(G.seed_of("fan" + layout))
    if layout == "contiguous":
        return B.leaf(G.ints(g, (2, 2, 3, 4, 4)), "const").requires_grad_(True)
    return B.leaf(G.ints(g, (2, 3, 2, 4, 4)), "const").permute(0, 2, 1, 3, 4).requires_grad_(True)      # (B, T, C, H, W) memory viewed as (B, C, T, H, W)


def _fan_case(B, layout, t, n_full, live):
    """`live`: which of (frame, full 1 .. full n) deliver a gradient"""
    x = _fan_x(B, layout)
    outs = B.fan_out(x, t, n_full)
    g = torch.Generator().manual_seed(G.seed_of(f"fan-cot:{layout}:{t}:{n_full}"))
    cots = [B.cot(G.ints(g, tuple(o.shape))) for o in outs]
    roots = [o if l else _Drop.apply(o) for o, l in zip(outs, live)]
    torch.autograd.backward(roots, cots)
    return None if x.grad is None else B.value(x.grad)


@pytest.mark.parametrize("layout", ["contiguous", "permuted"])
def test_fan_out(dev, rec, layout):
    from dcvgan_amd import native
    n = 0
    for t, n_full in itertools.product((0, 1, 2), (1, 2, 3)):
        for live in itertools.product((True, False), repeat=n_full + 1):
            fulls = sum(live[1:])
            rec.reset()
            if fulls == 0 and live[0]:
                with pytest.raises(native.NativeError, match="only the frame consumer delivered a gradient"):
                    _fan_case(G.Device(dev), layout, t, n_full, live)
                continue
            got = _fan_case(G.Device(dev), layout, t, n_full, live)
            c = rec.launches()
            if fulls == 0:
                assert got is None and not c, (live, c)
                continue
            want = _fan_case(G.Host(), layout, t, n_full, live)
            bad = G.mismatch(f"fan_out {layout} t={t} n_full={n_full} live={live}", got, want)
            assert not bad, bad
            assert c == Counter({"dcv_axpby": max(1, fulls - 1) + int(live[0])}), (live, c)
            WORDS[0] += want.numel()
            n += 1
    assert n == 3 * 2 * (1 + 3 + 7)


@pytest.mark.parametrize("L", [2, 3, 5])
def test_temporal_diff(dev, rec, L):
    res = []
    for B in (G.Device(dev), G.Host()):
        g = torch.Generator().manual_seed(G.seed_of(f"tdiff{L}"))
        x = B.leaf(G.ints(g, (2, 3, L, 4, 4)), "input")
        rec.reset()
        y = B.temporal_diff(x)
        y.backward(B.cot(G.ints(g, tuple(y.shape))))
        if isinstance(B, G.Device):
            assert rec.launches() == Counter({"dcv_axpby": 1 + 2 + int(L > 2)}), rec.launches()
        res.append(OrderedDict(y=B.value(y), dx=B.value(x.grad)))
    compare(f"temporal_diff L={L}", *res)


def test_cat_and_copy_into_strided(dev, rec):
    """cat_channels of a channel slice and a step-2 view; copy_into of a transposed view into a buffer slice, joined with a convolution's output"""
    res = []
    for B in (G.Device(dev), G.Host()):
        g = torch.Generator().manual_seed(G.seed_of("cat-copy"))
        wide = B.leaf(G.ints(g, (2, 7, 4, 6)), "input")
        step = B.leaf(G.ints(g, (2, 3, 4, 12)), "input")
        tr = B.leaf(G.ints(g, (2, 4, 6, 4)), "input")
        w = B.leaf(G.ternary(g, (8, 5, 3, 3), 0.3), "param")
        rec.reset()
        c = B.cat_channels(wide[:, 2:4], step[..., ::2])                  # (2, 5, 4, 6)
        buf = B.buffer(2, 8, 4, (4, 6))
        a = B.conv(c, w, (1, 1), (1, 1), out=(buf, "first"))
        z = B.copy_into(tr.transpose(2, 3), buf, "second")
        y = B.join(buf, a, z)
        y.backward(B.cot(G.ints(g, (2, 12, 4, 6))))
        if isinstance(B, G.Device):
            assert rec.launches() == Counter({"dcv_axpby": 3, "dcv_conv_forward": 1, "dcv_conv_backward_data": 1, "dcv_conv_backward_weight": 1}), rec.launches()
        res.append(OrderedDict(y=B.value(y), dwide=B.value(wide.grad), dstep=B.value(step.grad), dtr=B.value(tr.grad), dw=B.value(w.grad)))
    assert all(G.is_f32(t) for t in res[1].values())
    compare("cat / copy_into", *res)


def test_loss_sums_half_cotangent(dev, rec):
    """gan_loss_sum over a term that needs a gradient and one that does not, summed with a second loss by sum_scalars, upstream cotangent 1/2"""
    res = []
    for B in (G.Device(dev), G.Host()):
        g = torch.Generator().manual_seed(G.seed_of("loss-sums"))
        y1, y2, y3 = B.leaf(G.ints(g, (2, 8, 4, 4)), "input"), B.leaf(G.ints(g, (2, 8, 4, 4)), "const"), B.leaf(G.ints(g, (4, 4, 4)), "input")
        rec.reset()
        la = B.hinge_sum([(y1, G.KIND_HINGE_REAL), (y2, G.KIND_HINGE_FAKE)])
        lb = B.hinge_sum([(y3, G.KIND_HINGE_FAKE)])
        tot = B.sum_scalars(la, lb)
        tot.backward(B.cot(torch.tensor(0.5)))
        if isinstance(B, G.Device):
            # one scale per term that needs a gradient: y2 gets None and no launch
            assert rec.launches() == Counter({"dcv_gan_loss": 3, "dcv_axpby": 1, "dcv_scale_dev": 2}), rec.launches()
            assert y2.grad is None
        res.append(OrderedDict(la=B.value(la), lb=B.value(lb), tot=B.value(tot), dy1=B.value(y1.grad), dy3=B.value(y3.grad)))
    assert all(G.is_f32(t) for t in res[1].values())
    compare("loss sums", *res)


# ------------------------------------------------------------------------------------------------------------------------------------------------------
# the pack cache
# ------------------------------------------------------------------------------------------------------------------------------------------------------
def _pack_shapes():
    # (the smallest convolution here whose plan packs its weights is found by the test itself: it asserts that the cache holds an entry)
    return dict(n=2, cin=16, cout=64, sp=(16, 16))


def _conv_once(dev, w, x, cot):
    from dcvgan_amd import ops
    xx = x.detach().requires_grad_(True)
    y = ops.conv(xx, w, ops.conv_geom(w, (2, 2), (1, 1), False))
    (dx,) = torch.autograd.grad(y, [xx], cot)
    return y.detach().cpu(), dx.cpu()


def test_pack_cache_layouts_and_passes(dev, rec, monkeypatch):
    """One weight, two input layouts (contiguous, and a channel slice of a wider buffer), forward and data-gradient packs, visited alternately: every visit gives
    the twin's words, with the cache and without"""
    from dcvgan_amd import ops
    s = _pack_shapes()
    g = torch.Generator().manual_seed(G.seed_of("pack"))
    w64 = G.ternary(g, (s["cout"], s["cin"], 4, 4), 0.1)
    x64 = G.ints(g, (s["n"], s["cin"]) + s["sp"])
    cot64 = G.ints(g, (s["n"], s["cout"], s["sp"][0] // 2, s["sp"][1] // 2))
    xh = x64.clone().requires_grad_(True)
    yh = torch.nn.functional.conv2d(xh, w64, None, 2, 1)
    (dxh,) = torch.autograd.grad(yh, [xh], cot64)
    assert G.is_f32(yh.detach()) and G.is_f32(dxh) and float(torch.nn.functional.conv2d(x64.abs(), w64.abs(), None, 2, 1).max()) < G.LIMIT
    w = torch.nn.Parameter(w64.float().to(dev))
    xa = x64.float().to(dev)
    wide = torch.zeros((s["n"], s["cin"] + 3) + s["sp"], device=dev)
    wide[:, 3:] = xa
    xb = wide[:, 3:]
    cot = cot64.float().to(dev)
    visits = []
    for x in (xa, xb, xa, xb):
        y, dx = _conv_once(dev, w, x, cot)
        assert not G.mismatch("y", y, yh.detach()) and not G.mismatch("dx", dx, dxh)
        visits.append((y, dx))
    entries = w._dcv_pack.entries
    print(f"graph-exact pack cache: {len(entries)} entries, keys (which, strides) {[(k[0], k[4]) for k in entries]}")
    # a forward and a data-gradient pack per input layout: the strides are part of the key
    # a forward pack per input layout and the data-gradient pack (its dx is a fresh dense tensor either way): the strides are part of the key
    assert {(k[0], k[4]) for k in entries} == {(0, tuple(xa.stride())), (0, tuple(xb.stride())), (1, tuple(xa.stride()))} and len(entries) == 3, list(entries)
    assert tuple(xa.stride()) != tuple(xb.stride())
    with monkeypatch.context() as m:
        m.setattr(ops, "_USE_PACK_CACHE", False)
        w2 = torch.nn.Parameter(w64.float().to(dev))
        for x, (y0, dx0) in zip((xa, xb), visits):
            y, dx = _conv_once(dev, w2, x, cot)
            assert G.same_words(y, y0) and G.same_words(dx, dx0)
        assert getattr(w2, "_dcv_pack", None) is None
    WORDS[0] += 6 * (yh.numel() + dxh.numel())


@pytest.mark.parametrize("poison", [True, False], ids=["poison", "plain"])
def test_pack_cache_follows_adam_and_streams(dev, rec, monkeypatch, poison):
    """A step of the HIP Adam bumps the version: the next forward repacks and computes with the new values — the words of a fresh Parameter holding those values,
    which has no cache.  A forward on a side stream after the default stream packed gives the same words."""
    from dcvgan_amd import ops, optim
    monkeypatch.setattr(ops, "_POISON", poison)      # (poison adds a checksum of the live weights to the stamp: without it the version bump alone must cause the repack)
    s = _pack_shapes()
    g = torch.Generator().manual_seed(G.seed_of("pack-adam"))
    w = torch.nn.Parameter(G.ternary(g, (s["cout"], s["cin"], 4, 4), 0.2).float().to(dev))
    x = G.ints(g, (s["n"], s["cin"]) + s["sp"]).float().to(dev)
    geom = ops.conv_geom(w, (2, 2), (1, 1), False)
    with torch.no_grad():
        y0 = ops.conv(x, w, geom).cpu()
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        ys = ops.conv(x, w, geom)
    side.synchronize()
    assert G.same_words(ys.cpu(), y0)
    stamps = [e[0] for e in w._dcv_pack.entries.values()]
    assert stamps and all(st is not None for st in stamps)
    w.grad = G.ints(g, tuple(w.shape)).float().to(dev)
    v0 = w._version
    optim.Adam([w], lr=0.125).step()
    assert w._version > v0
    with torch.no_grad():
        y1 = ops.conv(x, w, geom).cpu()
        fresh = torch.nn.Parameter(w.detach().clone())
        y2 = ops.conv(x, fresh, geom).cpu()
    assert G.same_words(y1, y2) and not torch.equal(y1, y0)
    assert all(e[0] is not None and e[0][0] == w._version for e in w._dcv_pack.entries.values() if e[0] is not None)
    WORDS[0] += 2 * y0.numel()


def test_pack_stamp_is_cleared_until_commit(dev, rec):
    """A convolution call that fails after the cache handed out its buffer (here: the entry point is replaced by one that returns DCV_EWORKSPACE and launches nothing)
    never reaches commit(): the entry must not count as packed, and the retry packs again and gives the right words"""
    from dcvgan_amd import native, ops
    s = _pack_shapes()
    g = torch.Generator().manual_seed(G.seed_of("pack-commit"))
    w = torch.nn.Parameter(G.ternary(g, (s["cout"], s["cin"], 4, 4), 0.2).float().to(dev))
    x = G.ints(g, (s["n"], s["cin"]) + s["sp"]).float().to(dev)
    geom = ops.conv_geom(w, (2, 2), (1, 1), False)
    with torch.no_grad():
        y0 = ops.conv(x, w, geom).cpu()
    (e,) = w._dcv_pack.entries.values()
    assert e[0] is not None
    keep = rec._real

    class Failing:
        def __getattr__(self, n):
            return getattr(keep, n)

        def dcv_conv_forward(self, *a):
            return native.DCV_EWORKSPACE
    rec._real = Failing()
    try:
        with torch.no_grad(), pytest.raises(native.NativeError):
            ops.conv(x, w, geom)
    finally:
        rec._real = keep
    assert e[0] is None, "the entry still counts as packed after a call that never committed"
    with torch.no_grad():
        assert G.same_words(ops.conv(x, w, geom).cpu(), y0)
    assert e[0] is not None


def test_frozen_parameter_is_left_alone(dev, rec):
    """nn.Parameters with requires_grad False (a frozen BatchNorm, a frozen weight), with and without a .grad from before the freeze: the backward runs, nothing is
    added to that .grad and no accumulating entry is called"""
    from dcvgan_amd import ops
    o = XB.exact_operands("graph-frozen", (2, 8, 8, 8))
    f = lambda t: t.float().to(dev)
    for with_grad in (False, True):
        gamma, beta = torch.nn.Parameter(f(o.gamma), requires_grad=False), torch.nn.Parameter(f(o.beta), requires_grad=False)
        w = torch.nn.Parameter(f(G.ternary(torch.Generator().manual_seed(1), (8, 8, 3, 3), 0.2)), requires_grad=False)
        if with_grad:
            gamma.grad, beta.grad, w.grad = torch.ones_like(gamma), torch.ones_like(beta), torch.ones_like(w)
        x = f(o.x).requires_grad_(True)
        rec.reset()
        y = ops.conv(ops.bn_act(x, gamma, beta, None, None, True, ops.ACT_LEAKY, XB.SLOPE, eps=0.0), w, ops.conv_geom(w, (1, 1), (1, 1), False))
        y.backward(f(G.ints(torch.Generator().manual_seed(2), tuple(y.shape))))
        c = rec.launches()
        assert c["dcv_axpby"] == 0 and c["dcv_conv_backward_weight"] == 0 and c["dcv_conv_backward_weight_acc"] == 0 and c["dcv_bn_act_backward"] == 1, c
        for p in (gamma, beta, w):
            assert (p.grad is None) if not with_grad else bool((p.grad == 1).all())
        assert x.grad is not None and bool(torch.isfinite(x.grad).all())


def test_weight_changed_before_backward_raises(dev, rec):
    """An in-place change of the weight between a forward and its backward: autograd's saved-tensor check raises before anything is launched"""
    graph = G.GRAPHS["psum_s0.25"]
    B = G.Device(dev)
    L = graph.leaves(B)
    outs, _ = graph.fn(B, L)
    with torch.no_grad():
        L["w"].mul_(2.0)
    rec.reset()
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        torch.autograd.backward(outs, graph.cotangents(B))
    assert not rec.launches(), rec.launches()


# ------------------------------------------------------------------------------------------------------------------------------------------------------
# a BatchNorm group written with out= into the first slice, joined with a skip, read by a head convolution that carries its BnLink: the link must stay empty
# or be refused (this is no 64-wide 3-channel head), both nodes run their ordinary entries, gamma and beta go through deliver_small
# ------------------------------------------------------------------------------------------------------------------------------------------------------
BN_HEAD = ("plain_geometry", "transposed_small", "eval_mode", "dropout_mask", "other_stream")


def _bn_head_expected(variant):
    """fp64: exactbn's integer scheme for the BatchNorm input (a leaf, so that the group is exact), integers elsewhere"""
    import torch.nn.functional as F
    o = XB.exact_operands("graph-bn-head", (2, 8, 8, 8))
    g = torch.Generator().manual_seed(G.seed_of("bn-head" + variant))
    tr = variant == "transposed_small"
    w = G.ternary(g, (16, 3, 3, 3) if tr else (8, 16, 3, 3), 0.2)
    skip = G.ints(g, (2, 8, 8, 8))
    cot = G.ints(g, (2, 3 if tr else 8, 8, 8))
    mode = {"eval_mode": "eval", "dropout_mask": "dropout"}.get(variant, "leaky")
    r0 = XB.reference(o, mode, eps=0.0)
    buf = torch.cat([r0.y, skip], 1).requires_grad_(True)
    wl = w.clone().requires_grad_(True)
    y = (F.conv_transpose2d if tr else F.conv2d)(buf, wl, None, 1, 1)
    dbuf, dw = torch.autograd.grad(y, [buf, wl], cot)
    o = o._replace(dy=dbuf[:, :8].contiguous())
    r = XB.reference(o, mode, eps=0.0)
    assert XB.sums_exact(o, r, XB.RUN32, mode) and (mode == "eval" or XB.stats_exact(o, r))
    assert bool(XB.y_exact(o, r).all()), "the BatchNorm output is not exact"
    want = OrderedDict(y=y.detach(), dw=dw, dskip=dbuf[:, 8:].contiguous(), dgamma=r.dgamma, dbeta=r.dbeta)
    assert all(G.is_f32(t) for t in want.values())
    mag = (F.conv_transpose2d if tr else F.conv2d)(buf.detach().abs(), w.abs(), None, 1, 1)
    assert float(mag.max()) / G.grid_of(buf.detach()) < G.LIMIT
    return o, r, dict(w=w, skip=skip, cot=cot, mode=mode, tr=tr), want


def _bn_head_device(dev, variant, o, ops_, use_link):
    from dcvgan_amd import ops
    f = lambda t: t.float().to(dev)
    x = f(o.x).requires_grad_(True)
    gamma, beta = torch.nn.Parameter(f(o.gamma)), torch.nn.Parameter(f(o.beta))
    w, skip = torch.nn.Parameter(f(ops_["w"])), f(ops_["skip"]).requires_grad_(True)
    link = ops.BnLink() if use_link else None
    buf = ops.ConcatBuffer(2, 8, 8, (8, 8), dev)
    training = variant != "eval_mode"
    mask = f(o.mask).view(2, 8, 1, 1) if variant == "dropout_mask" else None
    rm, rv = (None, None) if training else (f(o.rm), f(o.rv))
    side = torch.cuda.Stream(dev) if variant == "other_stream" else None
    if side is not None:
        side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side if side is not None else torch.cuda.current_stream()):
        b = ops.bn_act(x, gamma, beta, rm, rv, training, ops.ACT_LEAKY, XB.SLOPE, mask=mask, eps=0.0, out=buf.first, link=link)
    if side is not None:
        torch.cuda.current_stream().wait_stream(side)
    z = ops.copy_into(skip, buf.second)
    y = ops.conv(buf.join(b, z), w, ops.conv_geom(w, (1, 1), (1, 1), ops_["tr"]), bn_link=link)
    y.backward(f(ops_["cot"]))
    torch.cuda.synchronize()
    c = lambda t: t.detach().cpu()
    return OrderedDict(y=c(y), dw=c(w.grad), dskip=c(skip.grad), dgamma=c(gamma.grad), dbeta=c(beta.grad)), c(x.grad)


@pytest.mark.parametrize("variant", BN_HEAD)
def test_bn_link_refused_or_empty(dev, rec, monkeypatch, variant):
    o, r, ops_, want = _bn_head_expected(variant)
    rec.reset()
    got, dx = _bn_head_device(dev, variant, o, ops_, True)
    c = rec.launches()
    print(f"graph-exact bn-head {variant}: {dict(sorted(c.items()))}")
    compare(f"bn head {variant}", got, want)
    # dx: word for word where exactbn proves it, within its counted bound elsewhere
    exact = XB.dx_exact(o, r) if ops_["mode"] != "eval" else torch.ones_like(r.dx, dtype=torch.bool)
    bound = torch.where(exact, torch.zeros_like(r.dx), XB.dx_bound(o, r))
    ratio = XB.assert_within(f"bn head {variant} dx", dx, r.dx, bound, (2, 8, 8, 8))
    print(f"graph-exact bn-head {variant}: dx exact at {int(exact.sum())} of {exact.numel()} elements, worst error / bound elsewhere {ratio:.3g}")
    assert ratio <= 1.0
    WORDS[0] += dx.numel()
    # both nodes on their ordinary entries; the fused entry either was not asked (empty link, other geometry, other stream) or refused
    # the BatchNorm node ran its own backward in every variant: nothing was fused.  The small transposed head passes the Python-side conditions and is handed to the
    # fused entry, which takes the data gradient and reports `fused = 0` (no 64-wide rows): the link stays empty
    asked = 1 if variant == "transposed_small" else 0
    assert c["dcv_bn_act_backward"] == 1 and c["dcv_conv_backward_weight"] == 1, c
    assert c["dcv_conv_backward_data_bn"] + c["dcv_conv_backward_data_bn!refused"] == asked and c["dcv_conv_backward_data"] + c["dcv_conv_backward_data_bn"] == 1, c
    assert c["dcv_bn_act_forward"] == 1 and c["dcv_conv_forward"] == 1 and not [k for k in c if "forward_bn" in k or "weight_bn" in k or "stats_only" in k], c
    plain, dx_plain = _bn_head_device(dev, variant, o, ops_, False)
    same(f"bn head {variant} link / no link", got, plain)
    assert G.same_words(dx, dx_plain)
    from dcvgan_amd import ops
    with monkeypatch.context() as m:      # the switch off: the link is not even looked at (no call of the fused entry), same words
        m.setattr(ops, "_HEAD_BN_FUSION", False)
        rec.reset()
        off, dx_off = _bn_head_device(dev, variant, o, ops_, True)
        assert not [k for k in rec.launches() if "data_bn" in k], rec.launches()
    same(f"bn head {variant} _HEAD_BN_FUSION off", got, off)
    assert G.same_words(dx, dx_off)


# ------------------------------------------------------------------------------------------------------------------------------------------------------
# the U-Net stage with a BatchNorm + ReLU group on the up path (out= into the first slice, gamma / beta through deliver_small): bounded, not exact
# ------------------------------------------------------------------------------------------------------------------------------------------------------
def _unet_bn_run(B, graph, pattern="once"):
    """-> results, launches; on top of the pattern's results the group's own quantities: its input u, output, cotangent and data gradient (tensor hooks)"""
    cap = {}
    L = graph.leaves(B)
    outs, taps = graph.fn(B, L)
    taps["bn_out"].register_hook(lambda g: cap.__setitem__("dy_bn", B.value(g)))
    taps["bn_in"].register_hook(lambda g: cap.__setitem__("dx_bn", B.value(g)))
    cap["u"], cap["y_bn"], cap["y"] = B.value(taps["bn_in"]), B.value(taps["bn_out"]), B.value(outs[0])
    torch.autograd.backward(outs, graph.cotangents(B), retain_graph=(pattern == "retain_twice"))
    G._grads(B, L, cap, "")
    if pattern == "retain_twice":
        torch.autograd.backward(outs, graph.cotangents(B))
        G._grads(B, L, cap, "second:")
    return cap


def test_unet_bn_within_exactbn_bounds(dev, rec):
    """The group's input u and its cotangent are integers on both sides (asserted word for word), so exactbn's counted bounds apply to y, dbeta, dgamma and dx with
    the operands (u, dy) — with two additions derived here, because the backward uses the DEVICE's saved statistics where exactbn's real-valued check hands it the
    reference's: with exactbn.stat_bounds' dmean (absolute, mean) and dis (relative, invstd), xhat moves by dxh = |is| dmean + |xhat| dis, hence
        dgamma = sum dz xhat      moves by  sum |dz| dxh                                              (the form of exactbn's Tanh term, ddz xhat)
        dx = g (dz - k0 - xhat k1), g = gamma is:  moves by  dis |dx| + |g| (dxh |k1| + |xhat| mean(|dz| dxh))     (g relative dis; xhat; k1 = mean(dz xhat))
    and dbeta = sum dz not at all.  dz is exact as long as no ReLU branch flips: asserted on the host (|z| above its own bound everywhere).  The stage's output adds
    the head's sum over 144 taps: |w4| * yb plus 145 U |w4| * |buffer| (any order of an fp32 sum of n terms: (n - 1) U sum |terms|, one rounding more for the store)."""
    import torch.nn.functional as F
    graph = G.unet_bn_graph()
    EPS, U = 1e-5, XB.U
    H = G.Host()
    want = _unet_bn_run(H, graph)
    rec.reset()
    got = _unet_bn_run(G.Device(dev), graph)
    c = rec.launches()
    assert c == graph.fwd + graph.bwd, c
    for k in ("u", "dy_bn"):
        bad = G.mismatch(k, got[k], want[k])
        assert not bad, bad
    vals = graph.values()
    o = XB.Operands(want["u"], want["dy_bn"], vals["gamma"], vals["beta"], None, None, None, None, None)
    r = XB.reference(o, "leaky", eps=EPS, slope=0.0)
    dims = (0, 2, 3)
    pc = lambda v: XB.per_channel(v, 4)
    bm, bv, dmean, dis, dvar = XB.stat_bounds(o, r, XB.RUN32, EPS)
    zb = XB.y_bound(o, r, dmean=dmean, dis_rel=dis, roundings=6)
    z = r.xh * pc(o.gamma) + pc(o.beta)
    assert bool((z.abs() > zb).all()), "a ReLU branch may flip: choose other operands"
    assert torch.allclose(r.y, want["y_bn"], rtol=0, atol=1e-12) and torch.allclose(r.dx, want["dx_bn"], rtol=0, atol=1e-9)      # exactbn's formulas are the twin's
    fig = {}
    shape = (2, 8, 8, 8)
    fig["y_bn"] = XB.assert_within("unet_bn y", got["y_bn"], r.y, zb, shape)
    dxh = pc(r.invstd.abs() * dmean) + r.xh.abs() * pc(dis)
    fig["dbeta"] = XB.assert_within("unet_bn dbeta", got["dbeta"], r.dbeta, (XB.RUN32 + 1) * U * r.dz.abs().sum(dims) + U * r.dbeta.abs(), shape)
    fig["dgamma"] = XB.assert_within("unet_bn dgamma", got["dgamma"], r.dgamma,
                                     (XB.RUN32 + 3) * U * (r.dz * r.xh).abs().sum(dims) + U * r.dgamma.abs() + (r.dz.abs() * dxh).sum(dims), shape)
    gi = pc((o.gamma * r.invstd).abs())
    dxb = XB.dx_bound(o, r, roundings=8, run=XB.RUN32) + pc(dis) * r.dx.abs() + gi * (dxh * pc(r.k1.abs()) + r.xh.abs() * pc((r.dz.abs() * dxh).mean(dims)))
    fig["dx_bn"] = XB.assert_within("unet_bn dx", got["dx_bn"], r.dx, dxb, shape)
    w4 = vals["w4"].abs()
    skip_mag = F.leaky_relu(F.conv2d(vals["x"], vals["w1"], None, 1, 1), 0.25).abs()
    yb = F.conv2d(torch.cat([zb, torch.zeros_like(skip_mag)], 1), w4, None, 1, 1) + 145 * U * F.conv2d(torch.cat([r.y.abs(), skip_mag], 1), w4, None, 1, 1)
    fig["y"] = XB.assert_within("unet_bn output", got["y"], want["y"], yb, shape)
    print("graph-exact unet_bn: worst error / bound " + " ".join(f"{k}={v:.3g}" for k, v in fig.items()))
    assert all(v < 1.0 for v in fig.values()), fig
    WORDS[0] += 4 * 1024 + 16
    # the gradients upstream of the group (w3, w2, w1, x) and w4's carry the group's rounding through three more layers; no counted bound is derived for them here:
    # they are held by the bit-identity tests below, and checked here only for being the twin's gradient at all (norm-relative, the ops suite's bar)
    for n in ("dx", "dw1", "dw2", "dw3", "dw4"):
        e = float((got[n].double() - want[n]).norm() / want[n].norm())
        assert e < 1e-5, (n, e)


@pytest.mark.parametrize("switch", ["_OWN_ACCUMULATION", "_WGRAD_SIDE"])
def test_unet_bn_call_patterns(dev, rec, monkeypatch, switch):
    """retain_graph twice: every gradient of the second pass is exactly twice the first (x + x is exact in fp32, whatever x), gamma and beta included (deliver_small's
    in-place add); the launches are the table's; and the accumulation routes ON and OFF agree bit for bit (same kernels, same operands, same order: one use per pass)"""
    from dcvgan_amd import ops
    graph = G.unet_bn_graph()
    rec.reset()
    on = _unet_bn_run(G.Device(dev), graph, "retain_twice")
    assert rec.launches() == graph.fwd + graph.bwd + graph.later(graph.bwd), rec.launches()
    for n in ("dx", "dw1", "dw2", "dw3", "dw4", "dgamma", "dbeta"):
        assert torch.equal(on["second:" + n], 2 * on[n]) and bool(torch.isfinite(on[n]).all()), n
    with monkeypatch.context() as m:
        m.setattr(ops, switch, False)
        off = _unet_bn_run(G.Device(dev), graph, "retain_twice")
    same(f"unet_bn retain_twice {switch}", on, off)


# ------------------------------------------------------------------------------------------------------------------------------------------------------
# the 16-bit channels-last path (ops_cl: its own ConcatBuffer, slot, gated call, companion): bf16 and fp16, exact — every stored tensor is held by both formats
# ------------------------------------------------------------------------------------------------------------------------------------------------------
CL_GRAPHS = OrderedDict((g.name, g) for g in (G.psum_cl_graph(), G.unet_cl_graph()))
CL_PATTERNS = ("once", "retain_twice", "pruned_first", "grad_beside_grads", "two_forwards_summed", "two_forwards_sequential")
CL_CASES = [(h, n, p) for h in ("bf16", "fp16") for n in CL_GRAPHS for p in CL_PATTERNS]


@functools.lru_cache(maxsize=None)
def twin_cl(name, pattern):
    return G.prove_cl(CL_GRAPHS[name], pattern)


def _cl_counts(c, half):
    """The path's convolution entries under the names of the fp32 table; the other element type's entries must not appear at all"""
    mine, other = ("dcv_clf16_", "dcv_cl_") if half == "fp16" else ("dcv_cl_", "dcv_clf16_")
    assert not [k for k in c if k.startswith(other) and not (other == "dcv_cl_" and k.startswith("dcv_clf16_"))], c
    g = lambda n: c[mine + n]
    return dict(fwd=g("conv_forward"), data=g("conv_backward_data") + g("conv_backward_data_gated"), gated=g("conv_backward_data_gated"),
                refused=g("conv_backward_data_gated!refused"), w=g("conv_backward_weight"), w_acc=g("conv_backward_weight_acc"))


@pytest.mark.parametrize("half,name,pattern", CL_CASES, ids=[f"{h}-{n}-{p}" for h, n, p in CL_CASES])
def test_cl_graph_against_twin(dev, rec, monkeypatch, half, name, pattern):
    """Exact: forward values, input gradients and the fp32 parameter gradients are the twin's words (tests/exactgraph.py::prove_cl: every tensor the path stores is a
    bf16 AND an fp16 value, |v| <= 256, so no store rounds; nothing here is merely bounded by half a 16-bit ulp).  The convolution entries, mark by mark, are those of
    the fp32 table under the path's names: first contributions by the plain weight-gradient entry, later ones by the accumulating one, none of either where
    torch.autograd.grad stands the in-place sums down; the U-Net's skip gradient by the path's own gated entry."""
    from dcvgan_amd import ops, ops_cl
    monkeypatch.setattr(ops_cl, "_HALF", [{"bf16": torch.bfloat16, "fp16": torch.float16}[half]])
    graph = CL_GRAPHS[name]
    got, marks = G.run_pattern(G.DeviceCL(dev), graph, pattern, rec)
    print(f"graph-exact cl {half} {name} {pattern}: {fmt(marks)}")
    compare(f"cl {half} {name} {pattern}", got, twin_cl(name, pattern))
    for (label, c), (label2, want) in zip(marks, G.expected_marks(graph, pattern)):
        assert label == label2
        k = _cl_counts(c, half)
        assert k["fwd"] == want["dcv_conv_forward"] and k["w"] == want["dcv_conv_backward_weight"] and k["w_acc"] == want["dcv_conv_backward_weight_acc"], (label, c)
        assert k["data"] == want["dcv_conv_backward_data"] + want["dcv_conv_backward_data_gated"] and k["gated"] == want["dcv_conv_backward_data_gated"] and not k["refused"], (label, c)
    if pattern == "retain_twice":
        for n, t in got.items():
            if n.startswith("second:"):
                assert torch.equal(t, 2 * got["first:" + n[7:]]), n
    if pattern == "grad_beside_grads":
        for n, t in got.items():
            if n.startswith("kept"):
                assert G.same_words(t, got["before:" + n.split(":")[1]]), n
    for mod, switch in ((ops, "_OWN_ACCUMULATION"), (ops, "_WGRAD_SIDE"), (ops_cl, "_WGRAD_SIDE"), (ops, "_SKIP_ACCUMULATE"), (ops, "_GATED_DGRAD")):
        with monkeypatch.context() as m:
            m.setattr(mod, switch, False)
            off, marks_off = G.run_pattern(G.DeviceCL(dev), graph, pattern, rec)
        same(f"cl {half} {name} {pattern} {mod.__name__}.{switch}", got, off)
        tot = sum((c for _, c in marks_off), Counter())
        if switch in ("_SKIP_ACCUMULATE", "_GATED_DGRAD"):
            assert not [k for k in tot if "gated" in k], tot
        if switch == "_OWN_ACCUMULATION":
            assert not [k for k in tot if k.endswith("weight_acc")], tot


class _SlottedCL(G.DeviceCL):
    """DeviceCL whose parameters carry a hand-set, NaN-filled `_dcv_grad_slot` (what optim.GradBucket hands its members under data parallelism)"""

    def __init__(self, device):
        super().__init__(device)
        self.slots = []

    def leaf(self, v, kind):
        t = super().leaf(v, kind)
        if kind == "param":
            t._dcv_grad_slot = torch.full(tuple(t.shape), float("nan"), device=self.device)
            self.slots.append((t, t._dcv_grad_slot))
        return t


@pytest.mark.parametrize("half", ["bf16", "fp16"])
def test_cl_weight_gradient_slot_rule(dev, rec, monkeypatch, half):
    """One rule for a weight's bucket slot on both paths (ops.deliver_wgrad): the first weight gradient of a backward is written into the slot whatever
    _OWN_ACCUMULATION says.  The CL16 parameter-sum graph, its weight used twice in one backward (real and fake batch): with the library's sums the second use is added
    into the slot by the accumulating entry and .grad IS the slot; without them the second use gets a tensor of its own from the plain entry and autograd adds.  The
    twin's words either way, and the same words (two exact terms: one sum)."""
    from dcvgan_amd import ops, ops_cl
    monkeypatch.setattr(ops_cl, "_HALF", [{"bf16": torch.bfloat16, "fp16": torch.float16}[half]])
    graph, pattern = CL_GRAPHS["psum_cl"], "two_forwards_summed"
    res = {}
    for own in (True, False):
        with monkeypatch.context() as m:
            m.setattr(ops, "_OWN_ACCUMULATION", own)
            B = _SlottedCL(dev)
            got, marks = G.run_pattern(B, graph, pattern, rec)
        compare(f"cl {half} slotted own={own}", got, twin_cl("psum_cl", pattern))
        (w, slot), = B.slots
        k = _cl_counts(dict(marks)["bwd_both"], half)
        assert (k["w"], k["w_acc"]) == ((1, 1) if own else (2, 0)) and k["data"] == 2 and not k["refused"], (own, marks)
        assert bool(torch.isfinite(slot).all()), "the slot was not written"
        if own:      # (where autograd's own sum ends up is autograd's business)
            assert w.grad.data_ptr() == slot.data_ptr() and G.same_words(slot.cpu(), got["dw"])
        res[own] = got
    same(f"cl {half} slotted _OWN_ACCUMULATION", res[True], res[False])


def test_zz_words_compared():
    print(f"graph-exact words compared: {WORDS[0]}")
