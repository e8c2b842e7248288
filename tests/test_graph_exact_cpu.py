"""CPU: the host half of the exact checks of the autograd plumbing (tests/exactgraph.py) — what tests/test_graph_exact_gpu.py relies on, checked without a GPU:
the twin's exactness claims for every (graph, pattern), the twin's graphs against torch.autograd.gradcheck, the recording proxy against a stub, and the case table."""
import json
import os
from collections import Counter, OrderedDict

import pytest
import torch

from tests import exactgraph as G

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "graph_cases.json")
CASES = [(n, p) for n in G.GRAPHS for p in (G.PATTERNS if n in G.PATTERN_GRAPHS else ("once",))]


@pytest.mark.parametrize("name,pattern", CASES, ids=[f"{n}-{p}" for n, p in CASES])
def test_twin_is_exact(name, pattern):
    """Every expected tensor is an fp32 value and no partial sum of any convolution can leave the 24-bit range on its grid (G.prove raises otherwise)"""
    res, worst = G.prove(G.GRAPHS[name], pattern, G.FROZEN.get(pattern, ()))
    assert res and 0.0 < worst < 1.0
    assert any(t is not None and bool((t != 0).any()) for n, t in res.items() if not n.startswith("y")) or pattern == "neither"


@pytest.mark.parametrize("pattern", ["once", "retain_twice", "pruned_first", "grad_beside_grads", "two_forwards_summed", "two_forwards_sequential"])
@pytest.mark.parametrize("make", [G.psum_cl_graph, G.unet_cl_graph], ids=["psum_cl", "unet_cl"])
def test_twin_is_exact_in_16_bits(make, pattern):
    """The channels-last cases: on top of the fp32 proof every stored tensor is a bf16 and an fp16 value with |v| <= 256 (G.prove_cl raises otherwise) — and the
    fp32 U-Net's operands are NOT, so the check is not vacuous"""
    assert G.prove_cl(make(), pattern)
    if pattern == "once":
        with pytest.raises(AssertionError, match="16-bit"):
            G.prove_cl(G.GRAPHS["unet_s0.25"], "once")


def test_augmented_segmentation_front_twin():
    """The fan_geometry variant of the segmentation front (kept out of GRAPHS: it has one call pattern): exact, and the twin's geometry-stream augmentation is the
    restatement of dcv_aug_apply (tests/test_augment_cpu.py::forward_ref) under the same rows, with x itself handed to the colour generator"""
    import numpy as np
    from tests.test_augment_cpu import forward_ref, make_table
    res, worst = G.prove(G.segmfront_graph(0.25, augmented=True), "once")
    assert 0.0 < worst < 1.0 and bool((res["dx"] != 0).any())
    x = G.ints(torch.Generator().manual_seed(3), (2, 3, 4, 8, 8))
    f, c, v, g = G.Host().fan_geometry(x, 1, G.SEGM_AUG_ROWS)
    want = torch.from_numpy(forward_ref(x.numpy().astype(np.float32), make_table(G.SEGM_AUG_ROWS), False)).double()
    assert c is x and v is g and torch.equal(v, want) and torch.equal(f, want[:, :, 1]) and not torch.equal(want, x)


def test_prove_rejects_inexact_operands():
    """A case that claims exactness it does not have fails on the host: thirds are on no binary grid, and 2^22-sized activations overflow 24 bits"""
    g = G.psum_graph(0.25)
    g.spec["x"] = (g.spec["x"][0], "input", lambda gen, s: G.ints(gen, s) / 3.0)
    with pytest.raises(AssertionError):
        G.prove(g, "once")
    g = G.psum_graph(0.25)
    g.spec["x"] = (g.spec["x"][0], "input", lambda gen, s: G.ints(gen, s) * 2.0 ** 22 + 1.0)
    with pytest.raises(AssertionError, match="not below 2\\^24|not an fp32"):
        G.prove(g, "once")


@pytest.mark.parametrize("name", list(G.GRAPHS))
def test_twin_against_gradcheck(name):
    """The Host build of every description under torch.autograd.gradcheck, fp64, real-valued operands (off the integer grid: away from the activations' kinks)"""
    graph = G.GRAPHS[name]
    gen = torch.Generator().manual_seed(G.seed_of("gradcheck" + name))
    kinds = graph.kinds()
    vals = OrderedDict((n, (torch.randn(v.shape, generator=gen, dtype=torch.float64) * 0.5)) for n, v in graph.values().items())
    names = [n for n in vals if kinds[n] != "const"]

    def f(*ts):
        L = dict(vals)
        L.update(zip(names, ts))
        return graph.fn(G.Host(exact=False), L)[0][0]
    assert torch.autograd.gradcheck(f, [vals[n].clone().requires_grad_(True) for n in names], fast_mode=True, eps=1e-6, atol=1e-5)


def test_host_elementwise_pieces_against_gradcheck():
    H = G.Host(exact=False)
    gen = torch.Generator().manual_seed(3)
    r = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64).requires_grad_(True)
    for L in (2, 3, 5):
        assert torch.autograd.gradcheck(H.temporal_diff, [r(2, 2, L, 3, 3)])
    assert torch.autograd.gradcheck(lambda x: sum((o * (i + 1)).sum() for i, o in enumerate(H.fan_out(x, 1, 2))), [r(2, 2, 3, 3, 3)])
    assert torch.autograd.gradcheck(lambda a, b: H.sum_scalars(H.hinge_sum([(a, G.KIND_HINGE_REAL), (b, G.KIND_HINGE_FAKE)]), a.sum()), [r(8) * 3, r(8) * 3])
    assert torch.autograd.gradcheck(lambda *a: H.gru(*a), [r(3, 2, 4), r(2, 4), r(12, 4), r(12, 4), r(12), r(12)])


def test_hinge_kinds_are_the_library_codes():
    import dcvgan_amd.ops as ops
    assert (G.KIND_HINGE_REAL, G.KIND_HINGE_FAKE) == (ops.KIND_HINGE_REAL, ops.KIND_HINGE_FAKE)
    from dcvgan_amd import native
    assert G.EUNSUPPORTED == native.DCV_EUNSUPPORTED


class _Stub:
    """Stands for the ctypes handle"""
    answer = 42

    def __init__(self):
        self.seen = []

    def dcv_conv_forward(self, a, b=0):
        self.seen.append(("fwd", a, b))
        return 0

    def dcv_conv_backward_data_gated(self, a):
        self.seen.append(("gated", a))
        return G.EUNSUPPORTED if a < 0 else 0

    def dcv_conv_workspace_bytes(self, a):
        return 4096

    def dcv_last_error(self):
        return b"text"

    def helper(self):
        return "not an entry point"


def test_recorder_forwards_and_records_in_order():
    stub = _Stub()
    rec = G.Recorder(stub)
    assert rec() is rec                                   # `lib()` returns the handle
    assert rec.dcv_conv_forward(7, b=3) == 0 and rec.dcv_conv_workspace_bytes(1) == 4096 and rec.dcv_last_error() == b"text"
    assert rec.dcv_conv_backward_data_gated(-1) == G.EUNSUPPORTED and rec.dcv_conv_backward_data_gated(5) == 0
    assert rec.helper() == "not an entry point" and rec.answer == 42
    assert stub.seen == [("fwd", 7, 3), ("gated", -1), ("gated", 5)]                   # arguments forwarded unchanged, every call made once
    assert rec.calls == ["dcv_conv_forward", "dcv_conv_workspace_bytes", "dcv_last_error", "dcv_conv_backward_data_gated!refused", "dcv_conv_backward_data_gated", "helper"]
    assert rec.launches() == Counter({"dcv_conv_forward": 1, "dcv_conv_backward_data_gated!refused": 1, "dcv_conv_backward_data_gated": 1})      # queries and helpers left out
    rec.reset()
    assert not rec.calls and not rec.launches()
    with pytest.raises(AttributeError):
        rec.dcv_no_such_entry


def test_recording_installs_and_restores():
    class Mod:
        pass
    a, b = Mod(), Mod()
    a.lib = b.lib = orig = (lambda: None)
    with pytest.raises(KeyError):
        with G.recording((a, b), _Stub()) as rec:
            assert a.lib is rec and b.lib is rec and a.lib().dcv_conv_forward(1) == 0
            raise KeyError("inside")
    assert a.lib is orig and b.lib is orig


def test_expected_launches_are_consistent():
    """The per-pattern expectations are sums of the table's forward / backward rows; `later` renames the weight-gradient entry and nothing else"""
    for g in G.GRAPHS.values():
        later = g.later(g.bwd)
        assert sum(later.values()) == sum(g.bwd.values()) and later["dcv_conv_backward_weight_acc"] == g.bwd["dcv_conv_backward_weight"] and "dcv_conv_backward_weight" not in later
        assert g.later(g.bwd, own=False) == g.bwd
        for p in G.PATTERNS:
            m = G.expected_marks(g, p)
            assert (m is None) == (p in G.FROZEN)
        assert set(g.late[1]) <= set(g.bwd) and g.late[0] in g.spec and g.spec[g.late[0]][1] == "param"


def test_case_table_is_pinned():
    """tests/golden/graph_cases.json: shapes and expected entry points per graph, and the routes — every route has a case that expects its entry point"""
    with open(GOLDEN) as fh:
        pinned = json.load(fh)
    table = json.loads(json.dumps(dict(cases=G.case_table(), routes={k: [v[0], list(v[1])] for k, v in G.ROUTES.items()}, patterns=list(G.PATTERNS))))
    assert table == pinned, "the case table changed: regenerate tests/golden/graph_cases.json on purpose (python -m tests.exactgraph) and say why in DESIGN 7e"
    for route, (entry, names) in G.ROUTES.items():
        assert names, route
        for n in names:
            g = G.GRAPHS[n]
            assert entry in g.bwd or entry in g.later(g.bwd), (route, n)
    for needed in ("dcv_conv_backward_data_gated", "dcv_conv_backward_data_gated!refused", "dcv_conv_backward_weight_acc", "dcv_conv_backward_weight"):
        assert any(needed == e for e, _ in G.ROUTES.values())
