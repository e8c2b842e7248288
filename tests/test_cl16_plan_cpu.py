"""CPU: the 16-bit channels-last convolutions plan before they launch (csrc/conv_cl16.hip: cl_plan, cl_wgrad_plan).

Sizes: every size query — packed weights and workspace of the forward and the data gradient, BatchNorm sums, weight-gradient workspace — of the bench-size layers
(tests/test_cl16_b100_gpu.py LAYERS), the six conv -> BatchNorm shapes of test_bn_sums_from_the_conv_epilogue_cl16 and a latent split-K layer, through the bf16
and the fp16 entry points, against tests/golden/cl16_plan_sizes.json.  That file was recorded from the library as it was BEFORE the planner existed (each query
with its own copy of the rules), with channels-last Dims5 of pitch pad8(c): a number that differs is a finding, not a reason to re-record.

Refusals: each one below is decided on the host before anything is launched (dcv_launch_count() counts attempts, and does not move)."""
import ctypes as C
import json
import os

import pytest

from tests.test_cl16_b100_gpu import LAYERS
from tests.test_cl16_gpu import test_bn_sums_from_the_conv_epilogue_cl16 as _bn_test

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "cl16_plan_sizes.json")
# Conv2d 256 -> 256, 4x4, stride 2, padding 1 on 4 x 256 x 4 x 4: one class, 128 K steps, 4 positions per sample = split-K x 8
LATENT = ("latent_conv_256_256", False, 256, 256, (4, 4), (2, 2), (1, 1), (4, 256, 4, 4))


def _t(v, n):
    return (v,) * n if isinstance(v, int) else tuple(v)


def cases():
    """(name, transposed, cin, cout, kernel, stride, padding, input shape), 2-D or 3-D"""
    out = [c[:8] for c in LAYERS]
    (mark,) = [m for m in _bn_test.pytestmark if m.name == "parametrize"]
    for name, tr, nd, cin, cout, k, s, p, sp, n in mark.args[1]:
        out.append(("bn_" + name, tr, cin, cout, _t(k, nd), _t(s, nd), _t(p, nd), (n, cin) + tuple(sp)))
    out.append(LATENT)
    assert len(out) == len(LAYERS) + 6 + 1 and len({c[0] for c in out}) == len(out)
    return out


def cl_dims(shape):
    """Dims5 of an (N, C, [D,] H, W) channels-last tensor with pixel pitch pad8(C)"""
    from dcvgan_amd.native import Dims5
    n, c = shape[0], shape[1]
    d, h, w = (1,) * (5 - len(shape)) + tuple(shape[2:])
    p = (c + 7) // 8 * 8
    return Dims5(n, c, d, h, w, d * h * w * p, 1, h * w * p, w * p, p)


def geom_and_dims(case):
    from dcvgan_amd.native import ConvGeom
    _, tr, cin, cout, k, s, p, xs = case
    k3, s3, p3 = (1,) * (3 - len(k)) + tuple(k), (1,) * (3 - len(s)) + tuple(s), (0,) * (3 - len(p)) + tuple(p)
    sp = (1,) * (5 - len(xs)) + tuple(xs[2:])
    out = tuple((i - 1) * st - 2 * pd + kk if tr else (i + 2 * pd - kk) // st + 1 for i, kk, st, pd in zip(sp, k3, s3, p3))
    g = ConvGeom(*k3, *s3, *p3, int(tr), cin, cout)
    return g, cl_dims(xs), cl_dims((xs[0], cout) + out[3 - len(k):])


def query_sizes(lib, prefix, case):
    g, xd, yd = geom_and_dims(case)
    f = lambda name: getattr(lib, prefix + name)
    a = (C.byref(g), C.byref(xd), C.byref(yd))
    return {"packed_bytes": [f("packed_bytes")(*a, 0), f("packed_bytes")(*a, 1)],
            "conv_workspace_bytes": [f("conv_workspace_bytes")(*a, 0), f("conv_workspace_bytes")(*a, 1)],
            "conv_stats_bytes": f("conv_stats_bytes")(*a),
            "wgrad_workspace_bytes": f("wgrad_workspace_bytes")(*a)}


@pytest.fixture(scope="module")
def lib():
    from dcvgan_amd import native
    if not os.path.exists(native.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return native.lib()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("prefix", ["dcv_cl_", "dcv_clf16_"])
@pytest.mark.parametrize("case", cases(), ids=lambda c: c[0])
def test_size_queries_are_what_they_were(lib, golden, case, prefix):
    want = golden[prefix][case[0]]
    got = query_sizes(lib, prefix, case)
    assert got == want, (case[0], got, want)
    assert min(got["packed_bytes"]) > 0 and min(got["conv_workspace_bytes"]) > 0 and got["wgrad_workspace_bytes"] > 0


# ---- refusals come before the first launch ----
PATCH_LAYER = ("convT_128_64", True, 128, 64, (4, 4), (2, 2), (1, 1), (2, 128, 16, 16))      # patch-staged: its tiles lie behind the tiled gather's in the pack
THIN_SRC = ("conv_3_32", False, 3, 32, (4, 4), (2, 2), (1, 1), (2, 3, 16, 16))                 # data gradient: 32 -> 3 channels, 48 GEMM columns = thin destination
THIN_DST = ("conv_256_1", False, 256, 1, (4, 4), (2, 2), (1, 1), (2, 256, 8, 8))               # forward: 256 -> 1 channel


@pytest.fixture()
def dummy():
    buf = C.create_string_buffer(4096)      # non-null, 16-byte aligned, never dereferenced by a call that is refused
    return (C.addressof(buf) + 15) // 16 * 16, buf


@pytest.mark.parametrize("prefix", ["dcv_cl_", "dcv_clf16_"])
def test_refusals_come_before_any_launch(lib, dummy, prefix):
    from dcvgan_amd import native as N
    p, _keep = dummy
    f = lambda name: getattr(lib, prefix + name)
    n0 = lib.dcv_launch_count()      # (0 where nothing else has run; a suite on a GPU has launched before)
    # (a) a pack buffer one byte short of the query, on a layer whose pack has the patch-staged tail
    g, xd, yd = geom_and_dims(PATCH_LAYER)
    a = (C.byref(g), C.byref(xd), C.byref(yd))
    nb = f("packed_bytes")(*a, 0)
    assert nb > 0
    assert f("pack_weights")(*a, 0, p, p, nb - 1, None) == N.DCV_EWORKSPACE, lib.dcv_last_error()
    # (b) the latent layer is split-K: without its slabs it is refused (it used to run unsplit: other bits)
    g, xd, yd = geom_and_dims(LATENT)
    assert f("conv_workspace_bytes")(C.byref(g), C.byref(xd), C.byref(yd), 0) == 256 + 8 * 128 * 256 * 4      # 8 splits x one 128-position tile x 256 channels, fp32
    assert f("conv_forward")(C.byref(g), p, C.byref(xd), p, p, C.byref(yd), 0, 0.0, p, 0, None) == N.DCV_EWORKSPACE, lib.dcv_last_error()
    assert b"split-K" in lib.dcv_last_error()
    assert f("conv_forward")(C.byref(g), p, C.byref(xd), p, p, C.byref(yd), 0, 0.0, None, 0, None) == N.DCV_EWORKSPACE
    # (c) no gated epilogue out of a thin source
    g, xd, yd = geom_and_dims(THIN_DST)      # its data gradient gathers dy: 1 channel
    ws = f("conv_workspace_bytes")(C.byref(g), C.byref(xd), C.byref(yd), 1)
    assert f("conv_backward_data_gated")(C.byref(g), p, C.byref(yd), p, p, C.byref(xd), 1, p, C.byref(xd), N.ACT_LEAKY, 0.2, p, ws, None) == N.DCV_EUNSUPPORTED, lib.dcv_last_error()
    # (d) a thin destination needs its Z tensor, forward (256 -> 1) and data gradient (32 -> 3) alike
    need = f("conv_workspace_bytes")(C.byref(g), C.byref(xd), C.byref(yd), 0)
    assert need == 2 * 8 * 8 * 32 * 2 + 512      # 128 source pixels x 16 taps x 1 channel (pitch 32), 16-bit
    assert f("conv_forward")(C.byref(g), p, C.byref(xd), p, p, C.byref(yd), 0, 0.0, p, need - 512 - 1, None) == N.DCV_EWORKSPACE, lib.dcv_last_error()
    g, xd, yd = geom_and_dims(THIN_SRC)
    assert f("conv_backward_data")(C.byref(g), p, C.byref(yd), p, p, C.byref(xd), 0, p, 64, None) == N.DCV_EWORKSPACE, lib.dcv_last_error()
    assert lib.dcv_launch_count() == n0


# ---- structure of the host half ----
def _host_half():
    lines = open(os.path.join(ROOT, "dcvgan_amd", "csrc", "conv_cl16.hip")).read().splitlines()
    start = lines.index("struct ClTile { int bn, bm; };")
    assert start == 1637      # the kernels above are not part of the host half
    return lines[start:]


def test_host_half_reads_its_switches_and_picks_its_tile_in_one_place():
    import re
    host = _host_half()
    ctor = [i for i, l in enumerate(host) if l.strip() == "ClToggles() {"]
    (acc,) = [i for i, l in enumerate(host) if l.startswith("static const ClToggles& cl_toggles()")]
    assert len(ctor) == 1 and ctor[0] < acc
    getenvs = [i for i, l in enumerate(host) if "getenv(" in l]
    assert getenvs and all(ctor[0] < i < acc for i in getenvs), "getenv outside ClToggles's constructor"
    # cl_pick_tile: its definition, and calls from cl_plan only
    (p0,) = [i for i, l in enumerate(host) if l.startswith("static int cl_plan(")]
    p1 = next(i for i in range(p0, len(host)) if host[i] == "}")
    calls = [i for i, l in enumerate(host) if re.search(r"\bcl_pick_tile\(", l) and not l.startswith("static ClTile cl_pick_tile(")]
    assert calls and all(p0 < i < p1 for i in calls), "cl_pick_tile called outside the planner"
    assert len(host) <= 765
