"""CPU: the host side of the exact-integer convolution checks (tests/exactconv.py, tests/test_conv_exact_gpu.py).

  * the reference checks itself: under the exactness bounds the fp32 host convolution equals the fp64 one bit for bit, for each host function the GPU rows use,
    and operands that break a bound are rejected before any device result would be looked at;
  * the gap the GPU tests close, demonstrated: one filter tap dropped at one border pixel of one sample is below every norm bar the suite holds convolutions to
    (1e-5 the tightest), and exactconv.first_mismatch names its coordinates;
  * no kernel form without an exact case: every kernel name the launchers can leave in dcv_debug_last_kernel's note is reached by a row of the GPU tables (by
    the notes recorded in tests/golden/conv_exact_notes.json), or is listed in NOT_EXACT with the reason — arithmetic that is not a sum of products.  A form
    added later fails here until it has a row."""
import json
import os
import re

import pytest
import torch
import torch.nn.functional as F

from tests import exactconv as X
from tests import test_conv_exact_gpu as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dcvgan_amd", "csrc")
S3, P3 = (1, 2, 2), (0, 1, 1)

# kernel forms whose arithmetic is not a sum of products (the only reason allowed here)
NOT_EXACT = {
    "head_bn_kernel": "the RGB head's data gradient fused with the BatchNorm backward, which divides by the element count: tests/test_rgb_head_gpu.py holds it to a tolerance",
}

SMALL = [X.case("self_conv2d", False, 2, 24, 40, 4, 2, 1, (12, 10), 3),
         X.case("self_convT2d", True, 2, 24, 20, 4, 2, 1, (6, 5), 3),
         X.case("self_conv3d", False, 3, 12, 24, 4, S3, P3, (5, 8, 8), 2),
         X.case("self_convT3d", True, 3, 6, 2, 4, S3, P3, (3, 4, 8), 2)]


@pytest.mark.parametrize("case", SMALL, ids=[c.name for c in SMALL])
def test_fp32_host_convolution_equals_fp64_under_the_bounds(case):
    r = X.reference(case)
    assert r["host_dtype"] == torch.float64
    X.assert_exactness_bounds(case, r, stats=True)
    x, w, dy = (r[k].clone() for k in ("x", "w", "dy"))
    x.requires_grad_(True); w.requires_grad_(True)
    y = X.conv_fn(case)(x, w, None, X._t(case.s, case.nd), X._t(case.p, case.nd))
    gx, gw = torch.autograd.grad((y * dy).sum(), [x, w])
    for got, key in ((y.detach(), "y"), (gx, "dx"), (gw, "dw")):
        assert got.dtype == torch.float32 and torch.equal(got.double(), r[key]), (case.name, key, X.first_mismatch(got, r[key]))
    # the derived quantities are what their definitions say, in fp64
    assert torch.equal(r["y_leaky"], torch.where(r["y"] > 0, r["y"], r["y"] * 0.25))
    assert torch.equal(r["dx_gated"], (r["old"].double() + r["dx"]) * torch.where(r["xg"] > 0, 1.0, 0.25))
    assert torch.equal(r["sum_y2"], (r["y"] ** 2).transpose(0, 1).flatten(1).sum(1))
    assert bool((r["y"] == r["y"].round()).all()) and float(r["y"].abs().max()) > 0


def test_operands_are_reproducible_from_the_case_name():
    a = X.int_operands((3, 4, 5), 3, 0.5, X.seed_of("some_case"))
    assert X.seed_of("some_case") == 2008806503 and torch.equal(a, X.int_operands((3, 4, 5), 3, 0.5, 2008806503))      # zlib.crc32: the same in every process
    assert bool((a == a.round()).all()) and float(a.abs().max()) <= 3 and 0.2 < float((a != 0).float().mean()) < 0.7


def test_a_case_that_breaks_a_bound_is_rejected():
    big = X.case("too_large_products", False, 2, 24, 40, 4, 2, 1, (12, 10), 3, 300)      # K * 300 * 300 = 384 * 90 000 > 2^24
    with pytest.raises(AssertionError):
        X.assert_exactness_bounds(big, X.reference(big))
    thin = X.case("z_beyond_bf16", False, 2, 256, 1, 4, 2, 1, (8, 8), 3, 8)               # Z of 256 channels of +-8 x +-8 leaves bf16's exact integers, not fp16's ... 
    r = X.reference(thin)
    X.assert_exactness_bounds(thin, r)
    assert 256 < X.thin_z(thin, r, 0) <= 2048
    X.assert_exactness_bounds(thin, r, half=torch.float16)
    with pytest.raises(AssertionError):
        X.assert_exactness_bounds(thin, r, half=torch.bfloat16)
    dense = X.case("sums_beyond_fp32", False, 2, 16, 40, 4, 2, 1, (64, 64), 96, 2)         # 98 304 positions of y^2 ~ 4000: the fused BatchNorm sums are not exact
    r = X.reference(dense)
    X.assert_exactness_bounds(dense, r)
    with pytest.raises(AssertionError):
        X.assert_exactness_bounds(dense, r, stats=True)


def test_a_dropped_border_tap_is_below_every_norm_bar_and_first_mismatch_finds_it():
    """The reason these files exist.  Conv2d 128 -> 256, 4x4 / 2 / 1 on 16 x 16, 96 samples (1.6 M outputs of rms ~90; the fp32 host convolution, exact under
    the bounds as the self-check above shows).  One tap of the filter, w[co, ci, kh, kw], zeroed at one border pixel of one sample changes one output by that one
    product: relative L2 below 1e-5, the tightest bar the suite holds convolutions to.  The same tap dropped for ALL input channels (a wrong halo test) is a
    difference of ~20 in one element: below the 1e-3 and 5e-3 bars.  Both are one differing element with known coordinates for first_mismatch."""
    case = X.case("gap_conv2d", False, 2, 128, 256, 4, 2, 1, (16, 16), 96)
    x = X.int_operands((case.n, case.cin) + case.sp, 2, 1.0, X.seed_of(case.name))
    w = X.int_operands(X.weight_shape(case), 2, 1.0, X.seed_of(case.name) + 1)
    assert case.cin * 16 * 2 * 2 < X.EXACT
    y = F.conv2d(x, w, None, 2, 1).double()
    n, co, oh, ow, kh, kw = 57, 200, 0, 5, 1, 2          # output row 0: a border pixel
    ih, iw = oh * 2 - 1 + kh, ow * 2 - 1 + kw
    prod = x[n, :, ih, iw].double() * w[co, :, kh, kw].double()
    ci = int((prod.abs() == 1).nonzero()[0])              # a channel whose product at that tap is +-1
    one = y.clone(); one[n, co, oh, ow] -= float(prod[ci])
    whole = y.clone(); whole[n, co, oh, ow] -= float(prod.sum())
    assert float(prod.sum()) != 0
    rel_one, rel_whole = float((one - y).norm() / y.norm()), float((whole - y).norm() / y.norm())
    print(f"relative L2 of one dropped (channel, tap) product: {rel_one:.2e}; of the tap dropped for all {case.cin} channels: {rel_whole:.2e}")
    assert 0 < rel_one < 1e-5, rel_one                    # below tests/test_b70_gpu.py's bar, and so below 1e-3 (test_ops_gpu.py) and 5e-3 (test_cl16_gpu.py)
    assert 0 < rel_whole < 1e-3, rel_whole
    for wrong in (one, whole):
        msg = X.first_mismatch(wrong, y)
        assert msg.startswith("1 of ") and "(n, c, d, h, w) = (57, 200, 0, 0, 5)" in msg, msg
        assert "on border rows/columns: 1" in msg and "on the last channel tile (c >= 128): 1" in msg and "on the last sample: 0" in msg, msg
        with pytest.raises(AssertionError, match=r"\(57, 200, 0, 0, 5\)"):
            X.assert_equal(wrong, y, "forward")
    assert X.first_mismatch(y, y) == ""


# ---- no form without an exact case ----
def kernel_names():
    names = set()
    mfma = open(os.path.join(CSRC, "conv_mfma.hip")).read()
    for m in re.finditer(r"DCV_NOTE_KERNEL\((.*)$", mfma, re.M):
        names.update(re.findall(r"\b(\w+_kernel)\b", m.group(1)))
    cl = open(os.path.join(CSRC, "conv_cl16.hip")).read()
    for m in re.finditer(r"snprintf\((?:P->note|g_last_kernel), sizeof\((?:P->note|g_last_kernel)\), (.*)$", cl, re.M):
        names.update(re.findall(r"\b(\w+_kernel)\b", m.group(1)))
    return names - {"g_last_kernel"}      # (the note's own buffer)


@pytest.fixture(scope="module")
def notes():
    with open(G.NOTES_PATH) as f:
        return json.load(f)


def test_every_kernel_form_has_an_exact_case(notes):
    names = kernel_names()
    assert {"gather_gemm_dma_kernel", "thin_rows_kernel", "head_bn_kernel", "wgrad_gemm_kernel", "thin_quad_kernel", "cl_gather_kernel", "cl_col2im_kernel",
            "cl_patch_convt_kernel", "cl_wgrad_kernel"} <= names and len(names) >= 24, sorted(names)      # the search itself still finds what it used to
    text = "\n".join(notes.values())
    missing = sorted(n for n in names if n not in NOT_EXACT and not re.search(r"\b" + n + r"\b", text))
    assert not missing, f"kernel forms without a row in tests/test_conv_exact_gpu.py: {missing}"
    assert set(NOT_EXACT) <= names and set(NOT_EXACT) == {"head_bn_kernel"}


def test_the_tables_and_the_recorded_notes_agree(notes):
    """Every call of every row has a recorded note, each row's `forms` hold in them, and nothing is recorded for a row that is gone."""
    keys = set()
    rows = [(row, str(m)) for row in G.FP32_ROWS for m in ((1, 2, 3) if row.lowp else (1,))] + [(row, h) for row in G.CL_ROWS for h in G.HALVES]
    assert len({row.name for row, _ in rows}) == len(G.FP32_ROWS) + len(G.CL_ROWS)
    for row, prec in rows:
        key = f"{row.name}|{prec}"
        mine = {k: v for k, v in notes.items() if k.startswith(key + "|")}
        assert mine, key
        keys.update(mine)
        for pas in row.forms:
            assert f"{key}|{pas}" in mine, (key, pas)
        for k, v in mine.items():
            for form in G.forms_of(row, k.split("|")[2], key):
                assert v == G.REFUSED or form in v, (k, form, v)
        if prec in ("2", "3"):      # the bf16-pipe instances say so
            assert any(G.PRECISION_NOTE[int(prec)] in v for v in mine.values()), key
        if prec in G.HALVES:
            assert all(("bf16" if prec == "bf16" else "fp16") + " channels-last" in v for v in mine.values() if v != G.REFUSED), key
    assert keys == set(notes)
