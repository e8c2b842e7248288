"""GPU: every convolution kernel form against the fp64 host convolution, bit for bit (tests/exactconv.py says why that is possible: small-integer operands make
every partial sum an integer below 2^24, so no order of summation, tiling, split-K or slab reduce may change a bit).  The norm-level bars of the other
convolution tests (1e-3 ... 1e-5) cannot see one dropped tap at one border pixel; here it is a non-zero integer at a known index, and the failure message
names the index (exactconv.first_mismatch).

One row of FP32_ROWS / CL_ROWS per kernel form, at the smallest shape the planners (plan_gather, plan_conv, plan_wgrad, cl_plan, cl_wgrad_plan) send there.
`forms` names, per pass, what the row is there for; tests/golden/conv_exact_notes.json holds the whole note (dcv_debug_last_kernel) of every call of every
row as the planners decide today.  A planner change that moves a row off its form fails here, and the CPU test (test_conv_exact_cpu.py) fails when a kernel
form has no row at all.  When a planner is changed on purpose: move the row by the planner's new rule so that `forms` still holds, then re-record the notes
(DCV_RECORD_CONV_NOTES=DIR writes what the run observed to DIR/conv_exact_notes.json, and the time of every case beside it).

Everything goes through the C ABI on the calling thread (the note is per thread, and autograd's backward runs on another).  Operands sit inside NaN-filled
allocations, outputs of non-accumulating calls are pre-filled with NaN (an element nobody wrote fails the equality), the workspace is exactly what the size
query says."""
import ctypes as C
import json
import os
import time

import pytest
import torch

from tests import exactconv as X

pytestmark = pytest.mark.gpu
GUARD = 4096                      # NaN elements on either side of every operand (a multiple of 4: the operand keeps its 16-byte alignment)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOTES_PATH = os.path.join(ROOT, "tests", "golden", "conv_exact_notes.json")
S3, P3 = (1, 2, 2), (0, 1, 1)
REFUSED = "DCV_EUNSUPPORTED"
PRECISION_NOTE = {1: "", 2: ", bf16 products", 3: ", f32x6: fp32 on the bf16 pipe"}


class Row:
    """case: the convolution and its operands.  forms: pass -> substring of the kernel note that the row exists for (passes: fwd, fwd_cl = forward on a
    channels-last-viewed input, dgrad, gated, wgrad, stats).  lowp: the forms have bf16-pipe instances (gather_gemm_dma_kernel, wgrad_dma_kernel): the row also runs
    with bf16 products and as f32x6.  misalign: operands start 4 bytes past a 16-byte boundary.  stats: 'direct' / 'none' = dcv_conv_forward_stats must / cannot
    leave BatchNorm partial sums."""

    def __init__(self, case, forms, lowp=False, misalign=0, stats=None):
        self.case, self.forms, self.lowp, self.misalign, self.stats = case, forms, lowp, misalign, stats
        self.name = case.name


c = X.case
# Forward / data-gradient forms first, then the weight-gradient forms; shapes of tests/test_ops_gpu.py CONVS, test_heads_gpu.py CASES, test_rgb_head_gpu.py
# HEAD_CASES and test_stem3d_wgrad_gpu.py CASES where those already reach a form.
FP32_ROWS = [
    # ---- gather_gemm_dma_kernel: tiles, patch staging, classes, walks, split-K ----
    Row(c("conv2d_4s2p1_16_oc24", False, 2, 12, 24, 4, 2, 1, (16, 16), 5), {"fwd": ("gather_gemm_dma_kernel<1, 2, 1, 4, false, true, ", "(32 x 256 tile, 1 class in"),
                                                                        "dgrad": "4 classes in one launch"}, lowp=True),
    Row(c("conv2d_4s2p1_32_oc40", False, 2, 8, 40, 4, 2, 1, (32, 32), 3), {"fwd": "(64 x 256 tile, 1 class in", "dgrad": "4 classes in one launch"}, lowp=True),
    Row(c("conv2d_4s2p1_32_oc130", False, 2, 6, 130, 4, 2, 1, (32, 32), 2), {"fwd": "(128 x 128 tile, 1 class in", "wgrad": "wgrad_gemm_kernel (128 x 128 tile"}, lowp=True),
    Row(c("conv2d_4s2p1_8_oc72", False, 2, 20, 72, 4, 2, 1, (8, 8), 7), {"fwd": "gather_gemm_dma_kernel", "wgrad": "wgrad_gemm_kernel (128 x 128 tile"}, lowp=True),
    # the halved tiles need 0.4 < rounds < 1 of the chip's 1024 workgroups at the full tile: 2 channel tiles x 256 position tiles = 0.5 (128 x 64), and
    # 1 x 512 (64 x 128)
    Row(c("conv2d_4s2p1_16_oc136_half", False, 2, 8, 136, 4, 2, 1, (16, 16), 512), {"fwd": "(128 x 64 tile, 1 class in"}, lowp=True),
    Row(c("conv2d_4s2p1_32_oc40_half", False, 2, 8, 40, 4, 2, 1, (32, 32), 512), {"fwd": "(64 x 128 tile, 1 class in"}, lowp=True),
    # no patch staging: an input row of 6 (not whole 16-byte granules), and operands 4 bytes past a 16-byte boundary
    Row(c("conv2d_4s2p1_6wide_oc24", False, 2, 12, 24, 4, 2, 1, (10, 6), 5), {"fwd": "gather_gemm_dma_kernel<1, 2, 1, 4, false, false, "}, lowp=True),
    Row(c("conv2d_4s2p1_16_oc24_unaligned", False, 2, 12, 24, 4, 2, 1, (16, 16), 5), {"fwd": "gather_gemm_dma_kernel<1, 2, 1, 4, false, false, "}, lowp=True, misalign=1),
    Row(c("convT2d_4s2p1_16_oc36", True, 2, 12, 36, 4, 2, 1, (16, 16), 3), {"fwd": "4 classes in one launch", "dgrad": "1 class in one launch"}, lowp=True),
    Row(c("convT2d_4s2p1_8_oc132", True, 2, 16, 132, 4, 2, 1, (8, 8), 5), {"fwd": "(128 x 128 tile, 4 classes in one launch"}, lowp=True),
    # walk 3 forward (4x4 inner taps, un-padded depth taps).  Its data gradient's depth taps leave the tensor, but the depth-step order also needs the gathered
    # channels (here cout) in whole groups of 4 (plan_gather: RC % 4 == 0): 70 channels stay on the 16-taps-per-step walk, so the depth-step rows have 72 and 36
    Row(c("conv3d_4s122_16_oc70", False, 3, 8, 70, 4, S3, P3, (6, 16, 16), 2), {"fwd": "gather_gemm_dma_kernel<2, 2, 2, 2, false, true, ",
                                                                             "dgrad": "gather_gemm_dma_kernel<1, 2, 1, 4, false, false, "}, lowp=True),
    Row(c("conv3d_4s122_16_oc72", False, 3, 8, 72, 4, S3, P3, (6, 16, 16), 2), {"fwd": "gather_gemm_dma_kernel<2, 2, 2, 2, false, true, ",
                                                                             "dgrad": "gather_gemm_dma_kernel<1, 2, 1, 4, true, true, "}, lowp=True),
    Row(c("conv3d_4s122_16_oc72_unaligned", False, 3, 8, 72, 4, S3, P3, (6, 16, 16), 2), {"dgrad": "gather_gemm_dma_kernel<1, 2, 1, 4, true, false, "}, lowp=True, misalign=1),
    Row(c("conv3d_4s122_32_oc36", False, 3, 8, 36, 4, S3, P3, (5, 32, 32), 2), {"fwd": "(64 x 256 tile", "dgrad": "gather_gemm_dma_kernel<1, 2, 1, 4, true, true, "}, lowp=True),
    Row(c("conv2d_4s2p1_wide", False, 2, 40, 72, 4, 2, 1, (8, 8), 5), {"fwd": ", split-K", "stats": "split-K"}, lowp=True, stats="none"),
    # ragged split-K, one class: 1280 tiles of 128 positions = one round + 256: k = 2, 8 K steps per part
    Row(c("conv2d_4s2p1_16_oc128_ragged", False, 2, 16, 128, 4, 2, 1, (16, 16), 2560, 1, 0.5), {"fwd": "1 class in one launch, ragged split-K"}, lowp=True),
    # ragged split-K, four-class data gradient: dy 128 channels on 8 x 8 -> dx 128 channels on 16 x 16, 1176 workgroups = one round + 152: k = 4
    Row(c("conv2d_4s2p1_16_c128_ragged_dgrad", False, 2, 128, 128, 4, 2, 1, (16, 16), 588, 1, 0.5), {"dgrad": "4 classes in one launch, ragged split-K",
                                                                                                  "gated": "4 classes in one launch, ragged split-K"}, lowp=True),
    # direct epilogue with BatchNorm partial sums: >= 384 workgroups.  Sparse +-1 operands keep sum y^2 per channel below 2^24 over 98 304 positions
    Row(c("conv2d_4s2p1_64_oc40_stats", False, 2, 16, 40, 4, 2, 1, (64, 64), 96, 1, 0.25), {"stats": "gather_gemm_dma_kernel", "fwd": "(64 x 256 tile"}, stats="direct"),
    # ---- the register-staged and the thin (OC <= 4) forms ----
    Row(c("conv2d_3s1p1", False, 2, 2, 6, 3, 1, 1, (12, 12), 2), {"fwd": "gather_gemm_kernel (", "dgrad": "thin_struct_kernel"}),
    Row(c("convT2d_3s1p1", True, 2, 8, 3, 3, 1, 1, (10, 10), 2), {"fwd": "thin_struct_kernel", "dgrad": "gather_gemm_kernel ("}),
    Row(c("conv2d_5s1p2_to2", False, 2, 6, 2, 5, 1, 2, (9, 11), 3), {"fwd": "thin_gather_kernel"}),
    Row(c("conv2d_2s2p0_to3", False, 2, 8, 3, 2, 2, 0, (10, 14), 3), {"fwd": "thin_struct_kernel"}),
    Row(c("conv2d_head", False, 2, 24, 1, 4, 2, 1, (8, 8), 4), {"fwd": "thin_struct_kernel", "dgrad": "head_dgrad_kernel<1>", "wgrad": "head_wgrad_kernel<1>"}),
    # thin_rows_kernel: kind 1 = 3x3 on 64-wide rows, 4 rows per image = one workgroup of 256 positions per image
    Row(c("convT2d_3s1p1_thin3_h4", True, 2, 12, 3, 3, 1, 1, (4, 64), 3), {"fwd": "thin_rows_kernel (OC 3, kind 1)"}),
    # kinds 2 and 3 (2x2 and 2x2x4 taps on 32-wide class rows) are the scatter classes of the 4x4 / stride-2 family to <= 4 channels, which thin_quad_kernel
    # takes first wherever the call may use it; the entry with BatchNorm sums may not, so it reaches them (and reports that it left no sums)
    Row(c("convT2d_4s2p1_to2", True, 2, 10, 2, 4, 2, 1, (32, 32), 6), {"fwd": "thin_quad_kernel<2, 1>", "stats": "thin_rows_kernel (OC 2, kind 2)"}, stats="none"),
    Row(c("convT3d_4s122_to1", True, 3, 6, 1, 4, S3, P3, (3, 8, 32), 2), {"fwd": "thin_quad_kernel<1, 4>", "stats": "thin_rows_kernel (OC 1, kind 3)"}, stats="none"),
    Row(c("conv2d_4s2p1_stem2", False, 2, 2, 8, 4, 2, 1, (64, 64), 4), {"dgrad": "thin_quad_kernel<2, 1>", "wgrad": "wgrad_gemm_kernel (128 x 32 tile"}),
    Row(c("conv3d_4s122_stem1", False, 3, 1, 8, 4, S3, P3, (9, 64, 64), 2), {"dgrad": "thin_quad_kernel<1, 4>"}),
    # widen_rows_kernel / widen_mfma_kernel: <= 4 gathered channels, 3x3 on 64-wide rows; 4 / 8 / 16 rows = 1 / 2 / 4 rows per wave
    Row(c("conv2d_3s1p1_from1_h4", False, 2, 1, 8, 3, 1, 1, (4, 64), 3), {"fwd": "widen_rows_kernel<1>"}),
    Row(c("conv2d_3s1p1_from2_h8", False, 2, 2, 96, 3, 1, 1, (8, 64), 2), {"fwd": "widen_rows_kernel<2>", "wgrad": "thin_wgrad3_kernel<2, 4>"}),
    Row(c("convT2d_3s1p1_head128_h4", True, 2, 128, 3, 3, 1, 1, (4, 64), 3), {"dgrad": "widen_mfma_kernel<3, 4>", "wgrad": "thinj_wgrad_kernel<3>"}),
    Row(c("convT2d_3s1p1_head64_h8", True, 2, 64, 3, 3, 1, 1, (8, 64), 2), {"dgrad": "widen_mfma_kernel<3, 2>"}),
    Row(c("convT2d_3s1p1_head256_h16", True, 2, 256, 3, 3, 1, 1, (16, 64), 1), {"wgrad": "thinj_wgrad_kernel<3>"}),
    Row(c("convT2d_3s1p1_head128_h2", True, 2, 128, 3, 3, 1, 1, (2, 64), 5), {"wgrad": "thinj_wgrad_kernel<3>"}),
    Row(c("convT2d_3s1p1_head128_h16", True, 2, 128, 3, 3, 1, 1, (16, 64), 2), {"dgrad": "widen_mfma_kernel<3, 4>"}),
    # ---- the discriminators' heads: plane counts that are no multiples of 4, 100 channels ----
    Row(c("conv3d_head_c100", False, 3, 100, 1, 4, S3, P3, (5, 8, 8), 3), {"fwd": "head_fwd_kernel<4>", "wgrad": "head_wgrad_kernel<4>"}),
    Row(c("conv2d_head_c100", False, 2, 100, 1, 4, 2, 1, (8, 8), 7), {"dgrad": "head_dgrad_kernel<1>", "wgrad": "head_wgrad_kernel<1>"}),
    # ---- weight-gradient forms ----
    # thin_wgrad3_kernel with a ragged last slab: N > 2048 / groups and N % pps != 0.  256 dense channels: 8 groups of 32 (one gathered channel) -> 257 images
    # in slabs of 2; 16 groups of 16 (two gathered channels) -> 129 images
    Row(c("conv2d_3s1p1_from1_oc256_n257", False, 2, 1, 256, 3, 1, 1, (4, 64), 257), {"wgrad": "thin_wgrad3_kernel<1, 8> (129 slabs)"}),
    Row(c("conv2d_3s1p1_from2_oc256_n129", False, 2, 2, 256, 3, 1, 1, (4, 64), 129), {"wgrad": "thin_wgrad3_kernel<2, 4> (65 slabs)"}),
    # stem3d_wgrad_kernel: row counts that are no multiple of the 8 rows a wave takes
    Row(c("conv3d_4s122_stem_c1_oc32", False, 3, 1, 32, 4, S3, P3, (5, 6, 64), 3), {"wgrad": "stem3d_wgrad_kernel<1, 2 stages>"}),
    Row(c("conv3d_4s122_stem_c2_oc32", False, 3, 2, 32, 4, S3, P3, (4, 10, 64), 1), {"wgrad": "stem3d_wgrad_kernel<2, 2 stages>"}),
    Row(c("conv3d_4s122_stem_c3_oc32", False, 3, 3, 32, 4, S3, P3, (6, 14, 64), 1), {"wgrad": "stem3d_wgrad_kernel<3, 2 stages>"}),
    # wgrad_dma_kernel: the 128 x 128 tile, the 64 x 128 tile with 16-byte staging of the dense operand, and without it (unaligned dense operand)
    Row(c("conv2d_4s2p1_wgrad_dma", False, 2, 16, 128, 4, 2, 1, (16, 16), 9), {"wgrad": ("wgrad_dma_kernel<2, ", "(128 x 128 tile")}, lowp=True),
    Row(c("convT2d_4s2p1_wgrad_dma", True, 2, 128, 8, 4, 2, 1, (8, 8), 21), {"wgrad": "wgrad_dma_kernel<2, "}, lowp=True),
    Row(c("conv3d_4s122_wgrad_dma", False, 3, 8, 128, 4, S3, P3, (6, 16, 16), 3), {"wgrad": "wgrad_dma_kernel<2, "}, lowp=True),
    Row(c("conv2d_4s2p1_wgrad_dma64", False, 2, 16, 64, 4, 2, 1, (16, 16), 9), {"wgrad": {1: "wgrad_dma_kernel<1, 0, true> (64 x 128 tile", 2: "wgrad_dma_kernel<1, 1, false> (64 x 128 tile", 3: "wgrad_dma_kernel<1, 0, true> (64 x 128 tile"}}, lowp=True),
    Row(c("conv2d_4s2p1_wgrad_dma64_unaligned", False, 2, 16, 64, 4, 2, 1, (16, 16), 9), {"wgrad": {1: "wgrad_dma_kernel<1, 0, false> (64 x 128 tile", 2: "wgrad_dma_kernel<1, 1, false> (64 x 128 tile", 3: "wgrad_dma_kernel<1, 0, false> (64 x 128 tile"}}, lowp=True, misalign=1),
    # wgrad_gemm_kernel, each tile of pick_wgrad_tile with the dense channels (DC) or the gathered channels x taps (J) one past a tile edge where the tile's rule allows
    Row(c("conv2d_4s2p1_dc129_j32", False, 2, 2, 129, 4, 2, 1, (8, 8), 2), {"wgrad": "wgrad_gemm_kernel (128 x 32 tile"}),
    Row(c("conv2d_4s2p1_dc129_j144", False, 2, 9, 129, 4, 2, 1, (8, 8), 2), {"wgrad": "wgrad_gemm_kernel (128 x 128 tile"}),
    Row(c("conv2d_3s1p1_dc129_j45", False, 2, 5, 129, 3, 1, 1, (8, 8), 2), {"wgrad": "wgrad_gemm_kernel (128 x 64 tile"}),
    Row(c("conv2d_4s2p1_dc40_j272", False, 2, 17, 40, 4, 2, 1, (8, 8), 2), {"wgrad": "wgrad_gemm_kernel (64 x 256 tile"}),
    Row(c("conv2d_4s2p1_dc40_j80", False, 2, 5, 40, 4, 2, 1, (8, 8), 2), {"wgrad": "wgrad_gemm_kernel (64 x 128 tile"}),
    Row(c("conv2d_3s1p1_dc192_j1152", False, 2, 128, 192, 3, 1, 1, (6, 6), 2), {"wgrad": "wgrad_gemm_kernel (64 x 128 tile"}),
    Row(c("conv2d_4s2p1_dc24_j272", False, 2, 17, 24, 4, 2, 1, (8, 8), 2), {"wgrad": "wgrad_gemm_kernel (32 x 256 tile"}),
    Row(c("conv2d_4s2p1_dc33_j80", False, 2, 5, 33, 4, 2, 1, (8, 8), 2), {"wgrad": "wgrad_gemm_kernel (64 x 128 tile"}),
    Row(c("conv2d_4s2p1_dc24_j80", False, 2, 5, 24, 4, 2, 1, (8, 8), 2), {"wgrad": "wgrad_gemm_kernel (32 x 128 tile"}),
    # ---- the segmentation configuration's own channel counts (CONFIGS["surreal-segm"]: 25 part maps, ggen 96, cgen 64, idis 64, vdis 48, gdis 32) ----
    # One row per geometry.  Each pass's note was probed once at the config's batch (60 clips = 960 frames, zero operands, no reference); the row has the smallest
    # probed n / depth whose notes name the same form and tile inside exactconv.FP64_BUDGET_MACS, and `forms` pins what was observed (slab counts aside).
    # ggen head, 960 x (32, 32): the tiles below; n = 24 / 32 still run the data gradient on another tile
    Row(c("segm_ggen_head_convT2d_96_25", True, 2, 96, 25, 4, 2, 1, (32, 32), 48), {"fwd": "(32 x 256 tile, 4 classes in one launch)", "dgrad": "(128 x 128 tile, 1 class in one launch)",
                                                                                 "gated": "(128 x 128 tile, 1 class in one launch)", "wgrad": "wgrad_gemm_kernel (128 x 128 tile"}),
    # cgen stem (Inconv, a reduction over 225), 960 x (64, 64): the register-staged form; n <= 16 runs the data gradient on another tile
    Row(c("segm_cgen_stem_conv2d_3s1p1_25_64", False, 2, 25, 64, 3, 1, 1, (64, 64), 24), {"fwd": "gather_gemm_kernel (64 x 256 tile)", "dgrad": "gather_gemm_kernel (32 x 256 tile)",
                                                                                       "gated": "gather_gemm_kernel (32 x 256 tile)", "wgrad": "wgrad_gemm_kernel (64 x 256 tile"}),
    # idis geometry stem, 60 x (64, 64): every n from 1 up leaves the batch's notes
    Row(c("segm_idis_stem_conv2d_4s2p1_25_32", False, 2, 25, 32, 4, 2, 1, (64, 64), 3), {"fwd": "(32 x 256 tile, 1 class in one launch, split-K)", "dgrad": "(32 x 256 tile, 4 classes in one launch)",
                                                                                      "gated": "(32 x 256 tile, 4 classes in one launch)", "wgrad": "wgrad_gemm_kernel (32 x 256 tile"}),
    # vdis / gdis geometry stems, 60 x (16 | 15, 64, 64).  The batch's forward runs WITHOUT split-K, which takes >= 98 304 output positions: 1.1e10 / 1.5e10 multiply-adds,
    # outside the budget.  No size inside it has that note; these rows have the batch's data-gradient and weight-gradient notes and the forward with split-K
    Row(c("segm_vdis_stem_conv3d_25_24", False, 3, 25, 24, 4, S3, P3, (4, 64, 64), 32), {"fwd": "(32 x 256 tile, 1 class in one launch, split-K)",
                                                                                      "dgrad": "gather_gemm_dma_kernel<1, 2, 1, 4, true, true, 0> (32 x 256 tile, 4 classes in one launch)",
                                                                                      "gated": "(32 x 256 tile, 4 classes in one launch)", "wgrad": "wgrad_gemm_kernel (32 x 256 tile"}),
    Row(c("segm_gdis_stem_conv3d_25_32", False, 3, 25, 32, 4, S3, P3, (4, 64, 64), 32), {"fwd": "(32 x 256 tile, 1 class in one launch, split-K)",
                                                                                      "dgrad": "gather_gemm_dma_kernel<1, 2, 1, 4, true, true, 0> (32 x 256 tile, 4 classes in one launch)",
                                                                                      "gated": "(32 x 256 tile, 4 classes in one launch)", "wgrad": "wgrad_gemm_kernel (32 x 256 tile"}),
    # vdis colour stem, 60 x (16, 64, 64): every probed size leaves the batch's notes (24 channels: not the 32-channel stem3d_wgrad_kernel; the gated entry is refused)
    Row(c("segm_vdis_stem_conv3d_3_24", False, 3, 3, 24, 4, S3, P3, (5, 64, 64), 3), {"fwd": "(32 x 256 tile, 1 class in one launch)", "dgrad": "thin_quad_kernel<3, 4>",
                                                                                   "wgrad": "wgrad_gemm_kernel (32 x 256 tile"}),
    # vdis trunk, 60 x (13, 32, 32) and 60 x (10, 16, 16).  At the batch: forward 128 x 128 with ragged split-K, data gradient 64 x 256 without split-K (48 -> 96);
    # data gradient 128 x 64 with ragged split-K (96 -> 192).  No probed size inside the budget keeps those (n = 32 at the full depth, 7.2e10 multiply-adds, still
    # differs): the smallest rows, which keep the forward's and the weight gradient's tiles and run everything with plain split-K
    Row(c("segm_vdis_trunk_conv3d_48_96", False, 3, 48, 96, 4, S3, P3, (6, 32, 32), 1), {"fwd": "(128 x 128 tile, 1 class in one launch, split-K)", "dgrad": "(64 x 256 tile, 4 classes in one launch, split-K)",
                                                                                      "gated": "(64 x 256 tile, 4 classes in one launch, split-K)", "wgrad": "wgrad_gemm_kernel (128 x 128 tile"}),
    Row(c("segm_vdis_trunk_conv3d_96_192", False, 3, 96, 192, 4, S3, P3, (6, 16, 16), 1), {"fwd": "(64 x 256 tile, 1 class in one launch, split-K)", "dgrad": "(128 x 128 tile, 4 classes in one launch, split-K)",
                                                                                        "gated": "(128 x 128 tile, 4 classes in one launch, split-K)", "wgrad": "wgrad_dma_kernel<1, 0, true> (64 x 128 tile"}),
    # vdis head, 60 x (7, 8, 8): every probed size leaves the batch's forms (the plane-group and share counts follow n)
    Row(c("segm_vdis_head_conv3d_192_1", False, 3, 192, 1, 4, S3, P3, (5, 8, 8), 3), {"fwd": "head_fwd_kernel<4>", "dgrad": "(64 x 256 tile, 4 classes in one launch)",
                                                                                   "gated": "(64 x 256 tile, 4 classes in one launch)", "wgrad": "head_wgrad_kernel<4>"}),
]
del c


def forms_of(row, pas, key):
    """the substrings row.forms asks of the note of pass `pas` (fwd.act, dgrad.acc and wgrad.acc run the form of fwd, dgrad, wgrad) at the precision / half type in `key`"""
    form = row.forms.get(pas.split(".")[0])
    if isinstance(form, dict):
        which = key.split("|")[1]
        form = form[int(which) if which.isdigit() else which]
    return () if form is None else (form,) if isinstance(form, str) else tuple(form)


# ---- plumbing ----
def _prod(shape):
    n = 1
    for v in shape:
        n *= v
    return n


class Guarded:
    """A tensor of `shape` (memory order `order`: a permutation of its dims, outermost first) inside a NaN-filled allocation"""

    def __init__(self, shape, dev, fill=None, dtype=torch.float32, shift=0, order=None):
        n = _prod(shape)
        self.big = torch.full((n + 2 * GUARD + shift,), float("nan"), dtype=dtype, device=dev)
        self.lo, self.hi = GUARD + shift, GUARD + shift + n
        body = self.big[self.lo:self.hi]
        if order is None:
            self.t = body.view(tuple(shape))
        else:
            inv = [order.index(i) for i in range(len(shape))]
            self.t = body.view(tuple(shape[i] for i in order)).permute(*inv)
        if fill is not None:
            self.t.copy_(fill)

    def intact(self):
        return bool(torch.isnan(self.big[:self.lo].float()).all() and torch.isnan(self.big[self.hi:].float()).all())


def geom_of(case, mfma=0):
    from dcvgan_amd.native import ConvGeom
    k, s, p = X._t(case.k, case.nd), X._t(case.s, case.nd), X._t(case.p, case.nd)
    k3, s3, p3 = (1,) * (3 - case.nd) + k, (1,) * (3 - case.nd) + s, (0,) * (3 - case.nd) + p
    return ConvGeom(*k3, *s3, *p3, int(case.tr), case.cin, case.cout, mfma)


class Judge:
    """What a run does with what it sees: the GPU tests assert; a planner probe without a GPU only records the notes."""

    def __init__(self, lib, notes, recorded, key):
        self.lib, self.notes, self.recorded, self.key = lib, notes, recorded, key

    def note(self, pas, row, text=None):
        text = self.lib.dcv_debug_last_kernel().decode() if text is None else text
        k = f"{self.key}|{pas}"
        self.recorded[k] = text
        for form in forms_of(row, pas, self.key):
            assert text == REFUSED or form in text, (k, "this row is here for", form, "but the call ran", text)
        assert self.notes.get(k) == text, (k, "recorded note", self.notes.get(k), "this run", text)
        return text

    def equal(self, got, want, what):
        X.assert_equal(got.double(), want.double(), f"{self.key} {what}")

    def equal16(self, got, want, what):
        """16-bit tensors as bit patterns"""
        assert got.dtype == want.dtype and got.element_size() == 2, (self.key, what, got.dtype, want.dtype)
        gi, wi = got.detach().cpu().contiguous().view(torch.int16), want.detach().cpu().contiguous().view(torch.int16)
        if not torch.equal(gi, wi):
            raise AssertionError(f"{self.key} {what}: {X.first_mismatch(got.float(), want.float())}")

    def true(self, cond, what):
        assert cond, f"{self.key}: {what}"

    def ok(self, rc, what):
        if rc == -3:      # DCV_EHIP: the runtime reported a fault; nothing more is started on the device from this module
            FAULTED.append(f"{self.key} {what}")
        assert rc == 0, (self.key, what, rc, self.lib.dcv_last_error())


@pytest.fixture(scope="module")
def dev():
    from dcvgan_amd import native
    native.lib()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def notes():
    with open(NOTES_PATH) as f:
        return json.load(f)


RECORDED = {}
TIMES = {}
FAULTED = []      # set by a HIP runtime error: the cases after it fail at once instead of launching onto a faulted device


def guarded_run(fn, *args):
    if FAULTED:
        pytest.fail(f"not run: the device reported a fault earlier in this module ({FAULTED[0]})")
    try:
        fn(*args)
        torch.cuda.synchronize()
    except RuntimeError as e:
        FAULTED.append(str(e)[:200])
        raise


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    out = os.environ.get("DCV_RECORD_CONV_NOTES")
    if out and os.path.isdir(out):
        with open(os.path.join(out, "conv_exact_notes.json"), "w") as f:
            json.dump(RECORDED, f, indent=0, sort_keys=True)
        with open(os.path.join(out, "conv_exact_times.json"), "w") as f:
            json.dump(TIMES, f, indent=0, sort_keys=True)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream) if torch.cuda.is_available() else None


def run_fp32(row, mfma, dev, J):
    """Every pass of one row at one precision.  J judges what is seen (Judge)."""
    from dcvgan_amd import native as N
    from dcvgan_amd.native import WPack, dims5, ptr
    L = J.lib
    cs = row.case
    r = X.reference(cs)
    X.assert_exactness_bounds(cs, r, stats=row.stats is not None)
    g = geom_of(cs, mfma)
    st = _stream()
    sh = row.misalign
    x = Guarded(r["x"].shape, dev, r["x"], shift=sh)
    w = Guarded(r["w"].shape, dev, r["w"], shift=sh)
    dy = Guarded(r["dy"].shape, dev, r["dy"], shift=sh)
    xm, ym = dims5(x.t), dims5(dy.t)
    need = [L.dcv_conv_workspace_bytes(C.byref(g), C.byref(xm), C.byref(ym), wh) for wh in (0, 1, 2)]
    ws = [torch.empty(max(nb, 1), dtype=torch.uint8, device=dev) for nb in need]
    eff = L.dcv_conv_effective_precision(C.byref(g))
    J.true(eff == mfma, f"effective precision {eff}")
    guards = [x, w, dy]

    def intact(what):
        J.true(all(gd.intact() for gd in guards), f"{what}: a NaN margin was written")

    # ---- forward: with a caller-owned pack (filled by the first call, read by the second), then on a channels-last-viewed input ----
    nb = L.dcv_conv_packed_bytes(C.byref(g), C.byref(xm), C.byref(ym), 0)
    pbuf = torch.empty(max(nb, 256), dtype=torch.uint8, device=dev)
    pack = WPack(pbuf.data_ptr(), nb, 0, eff)
    y = Guarded(r["y"].shape, dev)
    guards.append(y)
    J.ok(L.dcv_conv_forward(C.byref(g), ptr(x.t), C.byref(xm), ptr(w.t), ptr(y.t), C.byref(ym), N.ACT_NONE, 0.0, C.byref(pack) if nb else None, ptr(ws[0]), need[0], st), "forward")
    J.note("fwd", row)
    J.equal(y.t, r["y"], "forward")
    pack.ready = 1
    y.t.fill_(float("nan"))
    J.ok(L.dcv_conv_forward(C.byref(g), ptr(x.t), C.byref(xm), ptr(w.t), ptr(y.t), C.byref(ym), N.ACT_LEAKY, X.SLOPE, C.byref(pack) if nb else None, ptr(ws[0]), need[0], st), "forward + LeakyReLU")
    J.note("fwd.act", row)
    J.equal(y.t, r["y_leaky"], "forward + LeakyReLU(0.25), weights from the ready pack")
    nd5 = len(r["x"].shape)
    xcl = Guarded(r["x"].shape, dev, r["x"], order=[0] + list(range(2, nd5)) + [1])
    guards.append(xcl)
    xclm = dims5(xcl.t)
    need_cl = L.dcv_conv_workspace_bytes(C.byref(g), C.byref(xclm), C.byref(ym), 0)
    ws_cl = torch.empty(max(need_cl, 1), dtype=torch.uint8, device=dev)
    y.t.fill_(float("nan"))
    J.ok(L.dcv_conv_forward(C.byref(g), ptr(xcl.t), C.byref(xclm), ptr(w.t), ptr(y.t), C.byref(ym), N.ACT_NONE, 0.0, None, ptr(ws_cl), need_cl, st), "forward, channels-last view")
    J.note("fwd_cl", row)
    J.equal(y.t, r["y"], "forward on a channels-last-viewed input")
    intact("forward")
    # ---- forward with BatchNorm partial sums ----
    if row.stats is not None:
        sb = L.dcv_conv_stats_bytes(C.byref(g), C.byref(xm), C.byref(ym))
        stat = Guarded((max(sb // 4, 1),), dev)
        guards.append(stat)
        nparts, pitch = C.c_int(-1), C.c_int(-1)
        y.t.fill_(float("nan"))
        J.ok(L.dcv_conv_forward_stats(C.byref(g), ptr(x.t), C.byref(xm), ptr(w.t), ptr(y.t), C.byref(ym), ptr(stat.t), sb, C.byref(nparts), C.byref(pitch), None,
                                      ptr(ws[0]), need[0], st), "forward with sums")
        J.note("stats", row)
        J.equal(y.t, r["y"], "forward with BatchNorm sums")
        if dev.type == "cuda":
            if row.stats == "direct":
                J.true(nparts.value > 0 and pitch.value >= cs.cout and nparts.value * pitch.value * 8 <= sb, f"nparts {nparts.value}, pitch {pitch.value}, {sb} bytes")
                sums = stat.t[:nparts.value * pitch.value * 2].view(nparts.value, pitch.value, 2).double().sum(0).cpu()
                J.equal(sums[:cs.cout, 0], r["sum_y"], "sum y per channel")
                J.equal(sums[:cs.cout, 1], r["sum_y2"], "sum y^2 per channel")
                J.true(bool((sums[cs.cout:] == 0).all()), "padding channels of the sums read as zero")
            else:
                J.true(nparts.value == 0, f"nparts {nparts.value} from a form without a direct epilogue")
        intact("forward with sums")
    # ---- data gradient: plain, accumulated into a channel slice of a wider buffer, gated ----
    dx = Guarded(r["x"].shape, dev)
    guards.append(dx)
    J.ok(L.dcv_conv_backward_data(C.byref(g), ptr(dy.t), C.byref(ym), ptr(w.t), ptr(dx.t), C.byref(xm), 0, None, ptr(ws[1]), need[1], st), "data gradient")
    J.note("dgrad", row)
    J.equal(dx.t, r["dx"], "data gradient")
    extra = 5
    wide_shape = (cs.n, cs.cin + extra) + cs.sp
    wide_old = torch.cat([X.int_operands((cs.n, extra) + cs.sp, 8, 1.0, X.seed_of(cs.name) + 6), r["old"]], 1)
    wide = Guarded(wide_shape, dev, wide_old)
    guards.append(wide)
    sl = wide.t[:, extra:]
    slm = dims5(sl)
    need_sl = L.dcv_conv_workspace_bytes(C.byref(g), C.byref(slm), C.byref(ym), 1)
    ws_sl = torch.empty(max(need_sl, 1), dtype=torch.uint8, device=dev)
    J.ok(L.dcv_conv_backward_data(C.byref(g), ptr(dy.t), C.byref(ym), ptr(w.t), ptr(sl), C.byref(slm), 1, None, ptr(ws_sl), need_sl, st), "data gradient, accumulated")
    J.note("dgrad.acc", row)
    J.equal(sl, r["dx_acc"], "data gradient accumulated into a channel slice")
    J.equal(wide.t[:, :extra], wide_old[:, :extra], "the slice's neighbouring channels")
    xg = Guarded(r["xg"].shape, dev, r["xg"])
    guards.append(xg)
    xgm = dims5(xg.t)
    dx.t.copy_(r["old"])
    before = L.dcv_launch_count()
    rc = L.dcv_conv_backward_data_gated(C.byref(g), ptr(dy.t), C.byref(ym), ptr(w.t), ptr(dx.t), C.byref(xm), 1, ptr(xg.t), C.byref(xgm), N.ACT_LEAKY, X.SLOPE, None,
                                        ptr(ws[1]), need[1], st)
    if rc == N.DCV_EUNSUPPORTED:      # the thin (<= 4 destination channels) forms have no gated epilogue: refused before anything runs
        J.note("gated", row, REFUSED)
        J.true(min(cs.cin, 5) <= 4 and L.dcv_launch_count() == before, "a gated data gradient was refused by a form that has the epilogue, or after a launch")
        J.equal(dx.t, r["old"], "dx after a refused call")
    else:
        J.ok(rc, "gated data gradient")
        J.note("gated", row)
        J.equal(dx.t, r["dx_gated"], "gated, accumulated data gradient")
    intact("data gradient")
    # ---- weight gradient: plain, then accumulated onto an integer dw ----
    dw = Guarded(r["w"].shape, dev)
    guards.append(dw)
    J.ok(L.dcv_conv_backward_weight(C.byref(g), ptr(x.t), C.byref(xm), ptr(dy.t), C.byref(ym), ptr(dw.t), ptr(ws[2]), need[2], st), "weight gradient")
    J.note("wgrad", row)
    J.equal(dw.t, r["dw"], "weight gradient")
    dw.t.copy_(r["old_dw"])
    J.ok(L.dcv_conv_backward_weight_acc(C.byref(g), ptr(x.t), C.byref(xm), ptr(dy.t), C.byref(ym), ptr(dw.t), 1, ptr(ws[2]), need[2], st), "weight gradient, accumulated")
    J.note("wgrad.acc", row)
    J.equal(dw.t, r["dw_acc"], "accumulated weight gradient")
    intact("weight gradient")


def fp32_params():
    out = []
    for row in FP32_ROWS:
        for mfma in (1, 2, 3) if row.lowp else (1,):
            out.append(pytest.param(row, mfma, id=f"{row.name}-{('fp32', 'bf16', 'f32x6')[mfma - 1]}"))
    return out


@pytest.mark.parametrize("row,mfma", fp32_params())
def test_fp32_path_is_exact(dev, notes, row, mfma):
    from dcvgan_amd import native as N
    t0 = time.time()
    key = f"{row.name}|{mfma}"
    J = Judge(N.lib(), notes, RECORDED, key)
    guarded_run(run_fp32, row, mfma, dev, J)
    if mfma > 1:      # the bf16-pipe instances say so in the note of the passes whose form has one
        tagged = [k for k, v in RECORDED.items() if k.startswith(key + "|") and PRECISION_NOTE[mfma] in v]
        assert tagged, (key, "no pass ran a", PRECISION_NOTE[mfma], "instance")
    TIMES[key] = round(time.time() - t0, 2)
    print(f"{key}: {TIMES[key]} s (host reference {X.reference(row.case)['seconds']:.2f} s, {X.reference(row.case)['host_dtype']})")


# ---- the 16-bit channels-last path (dcv_cl_* in bf16, dcv_clf16_* in fp16) ----
# Shapes of tests/test_cl16_gpu.py CASES where they reach a form.  Operands of the thin-destination rows are sparse +-1: the form's 16-bit intermediate Z (a 1x1
# GEMM over up to 256 source channels) must itself be exact in 16 bits (exactconv.assert_exactness_bounds).
c = X.case
CL_ROWS = [
    # cl_gather_kernel: tiles, 1 class / 4 classes, thin source, split-K
    Row(c("cl_conv2d_4s2p1_64_128", False, 2, 64, 128, 4, 2, 1, (16, 16), 3), {"fwd": "cl_gather_kernel<128 x 128 tile> (1 class,", "wgrad": "cl_wgrad_kernel ("}, stats="direct"),
    Row(c("cl_conv2d_4s2p1_32_40", False, 2, 32, 40, 4, 2, 1, (32, 32), 2), {"fwd": "cl_gather_kernel<", "wgrad": "in pairs, 64 dense rows"}, stats="direct"),
    Row(c("cl_conv2d_4s2p1_96_192", False, 2, 96, 192, 4, 2, 1, (8, 8), 5), {"fwd": "cl_gather_kernel<"}),
    Row(c("cl_conv2d_4s2p1_thin3_32", False, 2, 3, 32, 4, 2, 1, (64, 64), 2), {"fwd": ", thin> (1 class,", "wgrad": "x 4 position splits"}),
    Row(c("cl_convT2d_4s2p1_64_64_h6w8", True, 2, 64, 64, 4, 2, 1, (6, 8), 2), {"fwd": "(4 classes,"}),      # a height the patch plan does not take: the tiled gather
    Row(c("cl_conv2d_4s2p1_256_256_latent", False, 2, 256, 256, 4, 2, 1, (4, 4), 4), {"fwd": "(1 class, split-K x 8,"}),
    Row(c("cl_convT2d_4s1p0_latent", True, 2, 50, 128, 4, 1, 0, (1, 1), 9), {"fwd": "cl_gather_kernel<"}),
    Row(c("cl_conv3d_4s122_64_128", False, 3, 64, 128, 4, S3, P3, (7, 16, 16), 2), {"fwd": "cl_gather_kernel<128 x 128 tile> (1 class,"}),
    # cl_patch_convt_kernel: 4-, 8-, 16- and 32-wide sources, an odd image count, 96 channels = 1.5 tiles
    Row(c("cl_convT2d_4s2p1_96_192_w4_n11", True, 2, 96, 192, 4, 2, 1, (4, 4), 11), {"fwd": ("cl_patch_convt_kernel<", "4 x 4 source")}, stats="direct"),
    Row(c("cl_convT2d_4s2p1_64_96_w8_n5", True, 2, 64, 96, 4, 2, 1, (8, 8), 5), {"fwd": ("cl_patch_convt_kernel<", "8 x 8 source")}),
    Row(c("cl_convT2d_4s2p1_128_64_w16", True, 2, 128, 64, 4, 2, 1, (16, 16), 3), {"fwd": ("cl_patch_convt_kernel<", "16 x 16 source")}),
    Row(c("cl_convT2d_4s2p1_32_64_w32", True, 2, 32, 64, 4, 2, 1, (32, 32), 2), {"fwd": ("cl_patch_convt_kernel<", "32 x 32 source")}),
    # thin destinations: the fused 3x3 form (images past a multiple of 8), and the 1x1 GEMM over the source + col2im
    Row(c("cl_convT2d_3s1p1_128_3_n9", True, 2, 128, 3, 3, 1, 1, (16, 64), 9, 1, 0.25), {"fwd": "cl_thin3x3_kernel<16>"}),
    Row(c("cl_convT2d_3s1p1_64_1_h32", True, 2, 64, 1, 3, 1, 1, (32, 64), 2, 1, 0.25), {"fwd": "cl_thin3x3_kernel<8>"}),
    Row(c("cl_convT2d_3s1p1_32_2", True, 2, 32, 2, 3, 1, 1, (16, 64), 3, 1, 0.5), {"fwd": "cl_thin3x3_kernel<4>"}),
    Row(c("cl_conv2d_4s2p1_256_1", False, 2, 256, 1, 4, 2, 1, (8, 8), 3, 1, 0.25), {"fwd": "as a 1x1 GEMM over the source + cl_col2im_kernel"}),
    Row(c("cl_convT2d_4s2p1_96_1", True, 2, 96, 1, 4, 2, 1, (32, 32), 2, 1, 0.25), {"fwd": "as a 1x1 GEMM over the source + cl_col2im_kernel"}),
    Row(c("cl_conv3d_4s122_256_1", False, 3, 256, 1, 4, S3, P3, (7, 8, 8), 2, 1, 0.25), {"fwd": "as a 1x1 GEMM over the source + cl_col2im_kernel"}),
    # thin sources: the fused 3-D stem and the fused 3x3 widening form
    Row(c("cl_conv3d_4s122_thin3_32", False, 3, 3, 32, 4, S3, P3, (5, 64, 64), 1), {"fwd": "cl_stem3d_kernel"}),
    Row(c("cl_conv3d_4s122_thin1_32_n3", False, 3, 1, 32, 4, S3, P3, (4, 64, 64), 3), {"fwd": "cl_stem3d_kernel"}),
    Row(c("cl_conv2d_3s1p1_thin1_64", False, 2, 1, 64, 3, 1, 1, (16, 64), 2), {"fwd": "cl_widen3x3_kernel<2>"}),
    Row(c("cl_conv2d_3s1p1_thin2_128_n9", False, 2, 2, 128, 3, 1, 1, (32, 64), 9), {"fwd": "cl_widen3x3_kernel<4>"}),
]
del c
HALVES = {"bf16": (torch.bfloat16, "dcv_cl_"), "f16": (torch.float16, "dcv_clf16_")}


class GuardedCl:
    """An (N, C, [D,] H, W) channels-last 16-bit tensor of pixel pitch `pitch` inside a NaN-filled allocation.  fill: the channels' values (the padding channels
    of the pixels are then zero, as every producer of such a tensor leaves them); None: all of it NaN, for a call to write."""

    def __init__(self, shape, dev, dtype, fill=None, pitch=None):
        from dcvgan_amd import ops_cl
        n, ch, sp = shape[0], shape[1], tuple(shape[2:])
        self.pitch = ops_cl.pitch_of(ch) if pitch is None else pitch
        numel = _prod((n,) + sp) * self.pitch
        self.big = torch.full((numel + 2 * GUARD,), float("nan"), dtype=dtype, device=dev)
        self.lo, self.hi = GUARD, GUARD + numel
        body = self.big[self.lo:self.hi].view((n,) + sp + (self.pitch,))
        perm = (0, len(sp) + 1) + tuple(range(1, len(sp) + 1))
        self.all = body.permute(*perm)
        self.t = self.all[:, :ch]
        if fill is not None:
            body.zero_()
            self.t.copy_(fill)

    def intact(self):
        return bool(torch.isnan(self.big[:self.lo].float()).all() and torch.isnan(self.big[self.hi:].float()).all())


def run_cl(row, half, dev, J):
    """Every pass of one channels-last row in one 16-bit type: outputs as bit patterns against the once-rounded reference, dw in fp32 exactly."""
    from dcvgan_amd import native as N
    from dcvgan_amd.native import dims5, ptr
    L = J.lib
    dtype, prefix = HALVES[half]
    f = lambda name: getattr(L, prefix + name)
    cs = row.case
    r = X.reference(cs)
    X.assert_exactness_bounds(cs, r, half=dtype, stats=row.stats is not None)
    once = lambda t: t.float().to(dtype)                      # the single rounding of an exact value
    g = geom_of(cs)
    st = _stream()
    x = GuardedCl(r["x"].shape, dev, dtype, r["x"])
    dy = GuardedCl(r["dy"].shape, dev, dtype, r["dy"])
    w = Guarded(r["w"].shape, dev, r["w"])
    xm, ym = dims5(x.t), dims5(dy.t)
    guards = [x, dy, w]
    c8 = lambda ch: (ch + 7) // 8 * 8

    def check16(gd, want, what):
        J.true(gd.t.dtype == dtype, "16-bit output")
        J.equal16(gd.t, once(want), what)
        ch = gd.t.shape[1]
        if c8(ch) > ch and dev.type == "cuda":
            J.true(bool((gd.all[:, ch:c8(ch)].float() == 0).all()), f"{what}: the channels between C and C rounded up to 8 are zero")
        J.true(all(q.intact() for q in guards), f"{what}: a NaN margin was written")

    def acc_want(note, gated):
        """dx_old + conv^T(dy, w) [, gated] as include/dcvgan_hip.h defines it per form: the tiled gather adds dx_old to the STORED (once-rounded) gradient, as a
        separate 16-bit add of two stored gradients would; the GEMM + col2im pair adds in fp32.  Either way every step is exact or one rounding of an exact value."""
        stored_first = note.startswith("cl_gather_kernel") and "cl_col2im_kernel" not in note
        v = r["old"].double() + (once(r["dx"]).double() if stored_first else r["dx"])
        return v * torch.where(r["xg"] > 0, 1.0, X.SLOPE).double() if gated else v

    packs = []
    for which in (0, 1):
        nb = f("packed_bytes")(C.byref(g), C.byref(xm), C.byref(ym), which)
        J.true(nb > 0, f"packed_bytes({which})")
        pk = torch.empty(max(nb, 1), dtype=torch.uint8, device=dev)
        J.ok(f("pack_weights")(C.byref(g), C.byref(xm), C.byref(ym), which, ptr(w.t), ptr(pk), nb, st), "pack_weights")
        packs.append(pk)
    need = [f("conv_workspace_bytes")(C.byref(g), C.byref(xm), C.byref(ym), wh) for wh in (0, 1)] + [f("wgrad_workspace_bytes")(C.byref(g), C.byref(xm), C.byref(ym))]
    ws = [torch.empty(max(nb, 1), dtype=torch.uint8, device=dev) for nb in need]
    # ---- forward, plain and with LeakyReLU(0.25) ----
    y = GuardedCl(r["y"].shape, dev, dtype)
    guards.append(y)
    J.ok(f("conv_forward")(C.byref(g), ptr(x.t), C.byref(xm), ptr(packs[0]), ptr(y.t), C.byref(ym), N.ACT_NONE, 0.0, ptr(ws[0]), need[0], st), "forward")
    J.note("fwd", row)
    check16(y, r["y"], "forward")
    y.all.fill_(float("nan"))
    J.ok(f("conv_forward")(C.byref(g), ptr(x.t), C.byref(xm), ptr(packs[0]), ptr(y.t), C.byref(ym), N.ACT_LEAKY, X.SLOPE, ptr(ws[0]), need[0], st), "forward + LeakyReLU")
    J.note("fwd.act", row)
    check16(y, r["y_leaky"], "forward + LeakyReLU(0.25)")
    # ---- forward with BatchNorm sums of the STORED values ----
    if row.stats is not None:
        y16 = once(r["y"]).double()
        red = tuple(i for i in range(y16.dim()) if i != 1)
        assert float(y16.abs().sum(red).max()) < X.EXACT and float((y16 * y16).sum(red).max()) < X.EXACT, (cs.name, "sums of the stored values")
        sb = f("conv_stats_bytes")(C.byref(g), C.byref(xm), C.byref(ym))
        stat = Guarded((max(sb // 4, 1),), dev)
        guards.append(stat)
        nparts, pitch = C.c_int(-1), C.c_int(-1)
        y.all.fill_(float("nan"))
        J.ok(f("conv_forward_stats")(C.byref(g), ptr(x.t), C.byref(xm), ptr(packs[0]), ptr(y.t), C.byref(ym), ptr(stat.t), sb, C.byref(nparts), C.byref(pitch), ptr(ws[0]), need[0], st),
             "forward with sums")
        J.note("stats", row)
        check16(y, r["y"], "forward with BatchNorm sums")
        if dev.type == "cuda":
            J.true(nparts.value > 0 and pitch.value >= cs.cout and nparts.value * pitch.value * 8 <= sb, f"nparts {nparts.value}, pitch {pitch.value}, {sb} bytes")
            sums = stat.t[:nparts.value * pitch.value * 2].view(nparts.value, pitch.value, 2).double().sum(0).cpu()
            J.equal(sums[:cs.cout, 0], y16.sum(red), "sum of the stored y per channel")
            J.equal(sums[:cs.cout, 1], (y16 * y16).sum(red), "sum of the stored y^2 per channel")
            J.true(bool((sums[cs.cout:] == 0).all()), "padding channels of the sums read as zero")
    # ---- data gradient: plain, accumulated, gated ----
    dx = GuardedCl(r["x"].shape, dev, dtype)
    guards.append(dx)
    J.ok(f("conv_backward_data")(C.byref(g), ptr(dy.t), C.byref(ym), ptr(packs[1]), ptr(dx.t), C.byref(xm), 0, ptr(ws[1]), need[1], st), "data gradient")
    J.note("dgrad", row)
    check16(dx, r["dx"], "data gradient")
    dxa = GuardedCl(r["x"].shape, dev, dtype, r["old"])
    guards.append(dxa)
    J.ok(f("conv_backward_data")(C.byref(g), ptr(dy.t), C.byref(ym), ptr(packs[1]), ptr(dxa.t), C.byref(xm), 1, ptr(ws[1]), need[1], st), "data gradient, accumulated")
    check16(dxa, acc_want(J.note("dgrad.acc", row), False), "accumulated data gradient")
    xg = GuardedCl(r["x"].shape, dev, dtype, r["xg"])
    guards.append(xg)
    dxa.t.copy_(r["old"])
    before = L.dcv_launch_count()
    rc = f("conv_backward_data_gated")(C.byref(g), ptr(dy.t), C.byref(ym), ptr(packs[1]), ptr(dxa.t), C.byref(xm), 1, ptr(xg.t), C.byref(xm), N.ACT_LEAKY, X.SLOPE, ptr(ws[1]), need[1], st)
    if rc == N.DCV_EUNSUPPORTED:      # the thin forms have no gated epilogue: refused before anything runs
        J.note("gated", row, REFUSED)
        J.true(min(cs.cin, cs.cout) <= 8 and L.dcv_launch_count() == before, "a gated data gradient was refused by a form that has the epilogue, or after a launch")
        J.equal16(dxa.t, once(r["old"]), "dx after a refused call")
    else:
        J.ok(rc, "gated data gradient")
        check16(dxa, acc_want(J.note("gated", row), True), "gated, accumulated data gradient")
    # ---- weight gradient (fp32), plain and accumulated ----
    dw = Guarded(r["w"].shape, dev)
    guards.append(dw)
    J.ok(f("conv_backward_weight")(C.byref(g), ptr(x.t), C.byref(xm), ptr(dy.t), C.byref(ym), ptr(dw.t), ptr(ws[2]), need[2], st), "weight gradient")
    J.note("wgrad", row)
    J.equal(dw.t, r["dw"], "weight gradient")
    dw.t.copy_(r["old_dw"])
    J.ok(f("conv_backward_weight_acc")(C.byref(g), ptr(x.t), C.byref(xm), ptr(dy.t), C.byref(ym), ptr(dw.t), 1, ptr(ws[2]), need[2], st), "weight gradient, accumulated")
    J.note("wgrad.acc", row)
    J.equal(dw.t, r["dw_acc"], "accumulated weight gradient")
    J.true(all(q.intact() for q in guards), "weight gradient: a NaN margin was written")


@pytest.mark.parametrize("half", list(HALVES))
@pytest.mark.parametrize("row", CL_ROWS, ids=[r.name for r in CL_ROWS])
def test_channels_last_path_is_exact(dev, notes, row, half):
    from dcvgan_amd import native as N
    t0 = time.time()
    key = f"{row.name}|{half}"
    guarded_run(run_cl, row, half, dev, Judge(N.lib(), notes, RECORDED, key))
    TIMES[key] = round(time.time() - t0, 2)
    print(f"{key}: {TIMES[key]} s (host reference {X.reference(row.case)['seconds']:.2f} s)")


def test_batchnorm_on_load_entries_are_exact(dev):
    """dcv_conv_forward_bn / dcv_conv_backward_weight_bn (the RGB head reading its BatchNorm's INPUT for the first cbn channels): gamma, invstd and the slope are
    powers of two, mean, beta and the BatchNorm input are integers, so act(x * gamma * invstd + beta - mean * gamma * invstd) is an integer however the kernel
    groups it, and the head's output and weight gradient must equal the host's on the materialised operand.  The plain operand's first cbn channels are NaN."""
    from dcvgan_amd import native as N
    from dcvgan_amd.native import dims5, ptr
    import torch.nn.functional as F
    L = N.lib()
    n, h, C_, cbn = 3, 8, 128, 64
    cs = X.case("bn_on_load_head", True, 2, C_, 3, 3, 1, 1, (h, 64), n)
    sd = X.seed_of(cs.name)
    bx = X.int_operands((n, cbn, h, 64), 2, 1.0, sd)
    mean, beta = X.int_operands((cbn,), 1, 1.0, sd + 1), 4 * X.int_operands((cbn,), 1, 1.0, sd + 2)
    gamma, invstd = torch.full((cbn,), 2.0), torch.full((cbn,), 2.0)
    gamma[::2] = 4.0; invstd[::2] = 1.0; gamma[1::4] = 8.0; invstd[1::4] = 0.5             # gamma * invstd = 4 in three ways
    rest = X.int_operands((n, C_ - cbn, h, 64), 2, 1.0, sd + 3)
    w = X.int_operands((C_, 3, 3, 3), 2, 1.0, sd + 4)
    dy = X.int_operands((n, 3, h, 64), 2, 1.0, sd + 5)
    old_dw = X.int_operands(w.shape, 8, 1.0, sd + 6)
    bc = lambda v: v.double()[None, :, None, None]
    z = bx.double() * bc(gamma * invstd) + bc(beta) - bc(mean) * bc(gamma * invstd)
    first = X.leaky(z)
    assert bool((first == first.round()).all()) and float(first.abs().max()) <= 24      # multiples of 4 before the slope of 1/4
    full = torch.cat([first, rest.double()], 1).requires_grad_(True)
    wr = w.double().requires_grad_(True)
    y_ref = F.conv_transpose2d(full, wr, None, 1, 1)
    (dw_ref,) = torch.autograd.grad((y_ref * dy.double()).sum(), [wr])
    y_ref = y_ref.detach()
    assert C_ * 9 * 24 * 2 < X.EXACT and n * h * 64 * 24 * 2 + 8 < X.EXACT                # the reduction bounds of the two passes
    holey = Guarded((n, C_, h, 64), dev)
    holey.t[:, cbn:] = rest.to(dev)
    gs = [holey] + [Guarded(t.shape, dev, t) for t in (bx, w, dy, gamma, beta, mean, invstd)]
    _, bxg, wg, dyg, gag, beg, meg, ing = gs
    y = Guarded(y_ref.shape, dev)
    dw = Guarded(w.shape, dev)
    gs += [y, dw]
    g = geom_of(cs, 1)
    xd, yd, bxd = dims5(holey.t), dims5(y.t), dims5(bxg.t)
    need = [L.dcv_conv_workspace_bytes(C.byref(g), C.byref(xd), C.byref(yd), wh) for wh in (0, 2)]
    ws = [torch.empty(max(nb, 1), dtype=torch.uint8, device=dev) for nb in need]
    tail = (cbn, ptr(bxg.t), C.byref(bxd), ptr(gag.t), ptr(beg.t), ptr(meg.t), ptr(ing.t), N.ACT_LEAKY, X.SLOPE)
    st = _stream()
    for act, want in ((N.ACT_NONE, y_ref), (N.ACT_LEAKY, X.leaky(y_ref))):
        y.t.fill_(float("nan"))
        N.check(L.dcv_conv_forward_bn(C.byref(g), ptr(holey.t), C.byref(xd), ptr(wg.t), ptr(y.t), C.byref(yd), act, X.SLOPE, None, ptr(ws[0]), need[0], *tail, st), "forward_bn")
        note = L.dcv_debug_last_kernel().decode()
        assert note == "thin_rows_kernel (OC 3, kind 1, BatchNorm + activation of the first 64 channels on load)", note
        X.assert_equal(y.t.double(), want, f"forward with BatchNorm on load, act {act}")
    for acc, want in ((0, dw_ref), (1, old_dw.double() + dw_ref)):
        dw.t.copy_(old_dw) if acc else dw.t.fill_(float("nan"))
        N.check(L.dcv_conv_backward_weight_bn(C.byref(g), ptr(holey.t), C.byref(xd), ptr(dyg.t), C.byref(yd), ptr(dw.t), acc, ptr(ws[1]), need[1], *tail, st), "backward_weight_bn")
        note = L.dcv_debug_last_kernel().decode()
        assert note.startswith("thinj_wgrad_kernel<3> (") and note.endswith("BatchNorm + activation of the first 64 dense channels on load)"), note
        X.assert_equal(dw.t.double(), want, f"weight gradient with BatchNorm on load, accumulate {acc}")
    assert all(q.intact() for q in gs)
