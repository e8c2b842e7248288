/*
 * dcvgan_hip.h — C ABI of libdcvgan_hip.so: the hand-written gfx950 (MI355X)
 * kernels under the DCVGAN generator/discriminator training step.
 *
 * The reference (raahii/dcvgan) is pure Python over torch.nn; it has no FFI of
 * its own.  Each entry point below replaces one torch.nn / torch.optim call
 * site of the reference's hot path (file:line given per function); the Python
 * host side (dcvgan_amd/native.py) binds them with ctypes — see INTEGRATION.md.
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer unless
 *     the name ends in _host; all tensors are fp32;
 *   - tensors are described as 5-D N,C,D,H,W sizes + element strides
 *     (2-D layers use D = 1), so the non-contiguous NCDHW views the reference
 *     produces (generator.py:139,433) are consumed without a copy;
 *   - `stream` is a hipStream_t passed as void*; nothing synchronises the host;
 *   - the caller owns every buffer, including `ws` scratch (size from the
 *     matching *_workspace_bytes call; 256-byte aligned);
 *   - return value: 0 on success, a negative DCV_E* code otherwise; nothing
 *     throws across the ABI.  dcv_last_error() gives a text for the last
 *     failure on the calling thread.
 *   - re-entrant: autograd runs backward kernels from its own thread.
 */
#ifndef DCVGAN_HIP_H
#define DCVGAN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DCV_OK 0
#define DCV_EINVAL (-1)   /* bad shape / geometry / null pointer          */
#define DCV_EWORKSPACE (-2) /* ws too small                                */
#define DCV_EHIP (-3)     /* a HIP runtime call failed                     */
#define DCV_EUNSUPPORTED (-4)

/* activation codes for fused epilogues / elementwise kernels */
#define DCV_ACT_NONE 0
#define DCV_ACT_LEAKY 1   /* LeakyReLU(slope); slope 0 = ReLU              */
#define DCV_ACT_TANH 2

typedef struct dcv_dims5 {
    int32_t n, c, d, h, w;        /* sizes                                  */
    int64_t sn, sc, sd, sh, sw;   /* element strides                        */
} dcv_dims5;

/* Geometry of one nn.Conv2d / nn.Conv3d / nn.ConvTranspose2d module.
 * cin/cout are the MODULE's in/out channels; weight layout is torch's:
 * (cout, cin, kd, kh, kw) for conv, (cin, cout, kd, kh, kw) for transposed. */
typedef struct dcv_conv_geom {
    int32_t kd, kh, kw;
    int32_t sd, sh, sw;
    int32_t pd, ph, pw;
    int32_t transposed;
    int32_t cin, cout;
    /* precision of the MFMA products for THIS module's three passes: 0 = the process default (dcv_set_precision), 1 = fp32, 2 = bf16 products,
     * 3 = fp32 emulated on the bf16 matrix pipe (each operand split into three bf16 pieces, 6 products, fp32 accumulation — see dcv_set_precision)
     * (a per-module switch; dcvgan_amd.util.set_precision(module, "bf16") sets it on a module's convolutions) */
    int32_t mfma;
} dcv_conv_geom;

const char* dcv_last_error(void);
/* ABI version.  Still 4: dcv_ema_update_multi was added without changing any struct or existing entry; likewise dcv_grad_guard_workspace_bytes, dcv_grad_guard_measure and dcv_adam_step_multi_guarded were added without changing any struct or existing entry.  4 (round 6): dcv_scale_dev, dcv_conv_backward_data_bn(_workspace_bytes), dcv_conv_forward_bn, dcv_conv_backward_weight_bn, dcv_bn_forward_stats_only, dcv_bn_apply exist (no struct changed).  3 (round 5): dcv_conv_backward_weight_acc / dcv_cl_conv_backward_weight_acc, dcv_cl_conv_backward_data_gated, dcv_clf16_*, dcv_normal_fill_many exist (no struct changed).
 * 2 (round 4): dcv_conv_geom has the 13th field `mfma`, dcv_wpack the 4th field `precision`, dcv_abi_struct_sizes exists.
 * A host compares dcv_version() and dcv_abi_struct_sizes() with its own declarations BEFORE the first call that passes a struct
 * (dcvgan_amd/native.py does, and refuses to load on a mismatch): the library cannot see the size of what a pointer points to. */
int dcv_version(void);
/* out[0..2] = sizeof(dcv_dims5), sizeof(dcv_conv_geom), sizeof(dcv_wpack) as this library was compiled */
void dcv_abi_struct_sizes(size_t out[3]);
/* number of kernel launches issued through this library so far (tests use it to
 * prove the HIP path, not a fallback, did the work) */
uint64_t dcv_launch_count(void);
/* DEFAULT precision of the MFMA products in the large GEMM kernels, for modules whose dcv_conv_geom.mfma is 0: 0 = fp32 (default; the mode every parity claim
 * and the headline benchmark refer to), 1 = bf16 products with fp32 accumulation (v_mfma_f32_32x32x16_bf16): tensors,
 * weights, BatchNorm statistics and optimiser state stay fp32, only the MFMA fragments are rounded (RNE) as they are read
 * from LDS.  A throughput mode for BASELINE.json's bf16 / fp16 configs; the reference itself is fp32-only. */
/* mode 2 (round 4, experimental, never the default): fp32 EMULATED on the bf16 matrix pipe.  Every fp32 operand is split exactly into three bf16 pieces
 * x = hi + mid + lo (RNE at each level); a bf16 x bf16 product is exact in fp32, and the six products of total order <= 2 (hi*hi, hi*mid, mid*hi, hi*lo, lo*hi,
 * mid*mid) are accumulated in fp32 by v_mfma_f32_32x32x16_bf16 — the dropped terms are <= 2^-23 of a product, the size of fp32's own rounding of it.  6 bf16
 * MFMAs (192 cycles) replace 8 fp32 ones (512 cycles) per 32 x 32 x 16 block; error against fp64 measured beside the native kernel's in profiles/r04_f32x6_*. */
int dcv_set_precision(int mode);
int dcv_get_precision(void);
/* the precision code (1 fp32, 2 bf16 products, 3 fp32-on-bf16) a dcv_conv_* call with this geometry would run at right now: g->mfma, or the process default
 * when that is 0.  A caller that owns packed weights (dcv_wpack) stamps them with it. */
int dcv_conv_effective_precision(const dcv_conv_geom* g);
/* diagnostics: which GEMM kernel instance the calling thread's last dcv_conv_* call launched (bench.py / tools label
 * their per-layer timings with it) */
const char* dcv_debug_last_kernel(void);
/* diagnostics text: resident workgroups/CU, registers, LDS of every GEMM kernel (needs a GPU) */
int dcv_debug_kernel_info(char* buf, size_t n);

/* ---- convolutions ------------------------------------------------------- *
 * Replace nn.Conv2d (generator.py:174,204; discriminator.py:83,89,95-101),
 * nn.Conv3d (discriminator.py:181-206,288-305) and nn.ConvTranspose2d
 * (generator.py:61-73,239-241,273-275) forward and their autograd backward.
 * Implicit GEMM on v_mfma_f32_32x32x2_f32.
 *   forward        : y = act(conv(x, w))            (act fused in the epilogue)
 *   backward_data  : dx (+)= conv^T(dy, w)
 *   backward_weight: dw  = corr(x, dy)              (deterministic split-K)
 */
size_t dcv_conv_workspace_bytes(const dcv_conv_geom* g, const dcv_dims5* x, const dcv_dims5* y, int which /*0 fwd,1 bwd-data,2 bwd-weight*/);
/* forward / backward_data read the weights K-major ("packed"); by default they re-pack them into `ws` on every call.
 * Weights only change at optimiser steps (trainer.py:320-322,357-359) while each layer runs 2-3 times per phase, so a
 * caller may own the packed copy instead: a buffer of dcv_conv_packed_bytes(g, x, y, which) bytes per (layer, which,
 * input geometry), passed with ready = 0 the first time after the weights changed (the call packs into it) and
 * ready = 1 afterwards (the packing launches are skipped).  pack = NULL keeps the default.
 * A packed copy is valid for ONE (weights, effective precision) pair — the packed FORMAT depends on the precision (fp32 [k][OCp]; bf16 products
 * [k/8][OCp][8] bf16; fp32-on-bf16: three such planes).  `precision` carries that pair's second half across the ABI: the caller sets it to
 * dcv_conv_effective_precision(g) when it hands the buffer over with ready = 0, keeps it with the buffer, and passes it back with ready = 1; a call whose
 * own effective precision differs from a ready pack's returns DCV_EINVAL before any launch (it never reads a pack of the other format), and a
 * ready = 0 call whose `precision` is not the call's own is refused the same way.  precision = 0 is refused too: there is no "unchecked" pack. */
typedef struct dcv_wpack {
    float* buf;
    size_t bytes;
    int32_t ready;
    int32_t precision;   /* 1 fp32, 2 bf16 products, 3 fp32-on-bf16: what `buf` was / is to be packed for */
} dcv_wpack;
size_t dcv_conv_packed_bytes(const dcv_conv_geom* g, const dcv_dims5* x, const dcv_dims5* y, int which /*0 fwd,1 bwd-data*/);
int dcv_conv_forward(const dcv_conv_geom* g, const float* x, const dcv_dims5* xd, const float* w,
                     float* y, const dcv_dims5* yd, int act, float slope, const dcv_wpack* pack,
                     void* ws, size_t ws_bytes, void* stream);
/* conv forward that also leaves per-tile BatchNorm partial sums of y (a conv -> BatchNorm pair, generator.py /
 * discriminator.py blocks): stat[part][pitch][2] = {sum, sum of squares}; *nparts = 0 when this geometry's
 * kernel cannot produce them (the caller then runs the plain statistics pass).  No activation, no accumulate. */
size_t dcv_conv_stats_bytes(const dcv_conv_geom* g, const dcv_dims5* x, const dcv_dims5* y);
int dcv_conv_forward_stats(const dcv_conv_geom* g, const float* x, const dcv_dims5* xd, const float* w, float* y, const dcv_dims5* yd,
                           float* stat, size_t stat_bytes, int* nparts, int* pitch, const dcv_wpack* pack, void* ws, size_t ws_bytes, void* stream);
int dcv_conv_backward_data(const dcv_conv_geom* g, const float* dy, const dcv_dims5* dyd, const float* w,
                           float* dx, const dcv_dims5* dxd, int accumulate, const dcv_wpack* pack,
                           void* ws, size_t ws_bytes, void* stream);
/* backward_data followed by the (Leaky)ReLU derivative of the layer that PRODUCED this conv's input, read off that
 * input itself: dx = (accumulate ? dx : 0) + conv^T(dy, w), then dx *= (x > 0 ? 1 : slope).  x must have dx's shape and
 * strides.  Replaces the separate derivative pass of an nn.Conv2d + nn.LeakyReLU pair whose output feeds this conv
 * (Inconv -> DownBlock 0, generator.py:173-176,203-207).  DCV_EUNSUPPORTED (before any launch) for geometries whose
 * kernels lack the gated epilogue: the caller then runs the two steps separately. */
int dcv_conv_backward_data_gated(const dcv_conv_geom* g, const float* dy, const dcv_dims5* dyd, const float* w,
                                 float* dx, const dcv_dims5* dxd, int accumulate,
                                 const float* x, const dcv_dims5* xd, int act, float slope, const dcv_wpack* pack,
                                 void* ws, size_t ws_bytes, void* stream);
/* A BatchNorm (+ activation) group whose output is NEVER WRITTEN (round 6; the colour generator's UpBlock 5, generator.py:238-250: 1.17 GB per pass at B = 70 that
 * only the RGB head reads): dcv_bn_forward_stats_only finalises the statistics the producing convolution's epilogue left (dcv_conv_forward_stats) and updates the running
 * statistics; the head's forward (dcv_conv_forward_bn) and weight gradient (dcv_conv_backward_weight_bn) then read the BatchNorm INPUT for the operand's first cbn
 * channels and apply act(x * gamma * invstd + beta - mean * gamma * invstd) on load, and dcv_conv_backward_data_bn (below) is the matching backward.
 * The *_bn conv entries take only the head's geometry (3x3 / 1 / 1, 3 output channels, 64-wide rows, fp32) and return DCV_EUNSUPPORTED for anything else BEFORE running
 * anything; a caller that gets that materialises the output with dcv_bn_apply and uses the plain entries. */
int dcv_bn_forward_stats_only(const float* x, const dcv_dims5* xd, float* running_mean, float* running_var, int64_t* num_batches_tracked, float* save_mean, float* save_invstd,
                              float momentum, float eps, const float* stat, int nparts, int pitch, void* stream);
int dcv_bn_apply(const float* x, const dcv_dims5* xd, float* y, const dcv_dims5* yd, const float* gamma, const float* beta, const float* save_mean, const float* save_invstd,
                 const float* mask, int act, float slope, void* stream);
int dcv_conv_forward_bn(const dcv_conv_geom* g, const float* x, const dcv_dims5* xd, const float* w, float* y, const dcv_dims5* yd, int act, float slope,
                        const dcv_wpack* pack, void* ws, size_t ws_bytes, int cbn, const float* bn_x, const dcv_dims5* bn_xd, const float* gamma, const float* beta,
                        const float* save_mean, const float* save_invstd, int bn_act, float bn_slope, void* stream);
int dcv_conv_backward_weight_bn(const dcv_conv_geom* g, const float* x, const dcv_dims5* xd, const float* dy, const dcv_dims5* dyd, float* dw, int accumulate,
                                void* ws, size_t ws_bytes, int cbn, const float* bn_x, const dcv_dims5* bn_xd, const float* gamma, const float* beta,
                                const float* save_mean, const float* save_invstd, int bn_act, float bn_slope, void* stream);
/* The data gradient of a convolution whose first `cbn` input channels are the output of a BatchNorm (training mode, no dropout mask) + (Leaky)ReLU | identity, FUSED
 * with that BatchNorm's backward — the last stage of the colour generator: `UpBlock` 5 -> torch.cat with the stem's skip -> `Outconv`
 * (generator.py:238-250,272-277,393-400).  Where the geometry is the RGB head's (3x3 / stride 1 / pad 1 transposed, 3 -> 128 channels on 64-wide rows, fp32) the gradient
 * of those cbn channels is never written: it is recomputed from dy inside the BatchNorm reduction and inside the kernel that writes the gradient of the BatchNorm INPUT
 * (4.7 GB of HBM traffic per call instead of 8.2 GB at B = 70).  On return *fused = 1: dx[:, cbn:] , bn_dx, dgamma, dbeta are written and dx[:, :cbn] is NOT;
 * *fused = 0: the plain data gradient ran (any other geometry), dx is complete and the caller runs dcv_bn_act_backward itself.  ws / pack: as dcv_conv_backward_data;
 * ws2: dcv_conv_backward_data_bn_workspace_bytes(dxd, cbn) bytes.  act: DCV_ACT_NONE or DCV_ACT_LEAKY (slope 0 = ReLU) of the BatchNorm group. */
size_t dcv_conv_backward_data_bn_workspace_bytes(const dcv_dims5* dxd, int cbn);
int dcv_conv_backward_data_bn(const dcv_conv_geom* g, const float* dy, const dcv_dims5* dyd, const float* w, float* dx, const dcv_dims5* dxd, const dcv_wpack* pack,
                              void* ws, size_t ws_bytes, int cbn, const float* bn_x, const dcv_dims5* bn_xd, const float* gamma, const float* beta,
                              const float* save_mean, const float* save_invstd, int act, float slope, float* bn_dx, const dcv_dims5* bn_dxd, float* dgamma, float* dbeta,
                              void* ws2, size_t ws2_bytes, int* fused, void* stream);
int dcv_conv_backward_weight(const dcv_conv_geom* g, const float* x, const dcv_dims5* xd,
                             const float* dy, const dcv_dims5* dyd, float* dw,
                             void* ws, size_t ws_bytes, void* stream);
/* dw = (accumulate ? dw : 0) + corr(x, dy)  (ABI 3).  Replaces the elementwise sums autograd forms when a weight is used twice in one backward (every discriminator
 * parameter: D on the real and on the fake batch, trainer.py:299-309 -> :319) or when .grad already holds an earlier backward's gradient (the discriminators in the
 * G phase, trainer.py:356 on top of :319; discriminator.zero_grad() only at :288-290): the slab reduce adds its fixed-order sum to dw — the same two operands and
 * one rounding as torch's add, so the result is bit-identical. */
int dcv_conv_backward_weight_acc(const dcv_conv_geom* g, const float* x, const dcv_dims5* xd,
                                 const float* dy, const dcv_dims5* dyd, float* dw, int accumulate,
                                 void* ws, size_t ws_bytes, void* stream);

/* ---- BatchNorm{2,3}d (+ Dropout2d) (+ activation) ------------------------ *
 * Replace nn.BatchNorm2d/3d + nn.Dropout2d + nn.(Leaky)ReLU chains
 * (generator.py:62-72,205-211,242-248; discriminator.py:96-100,191-202,290-302).
 * Training mode: batch statistics over (N, D, H, W), biased variance for the
 * normalisation, unbiased for running_var, momentum 0.1 (torch defaults).
 *   y = act( mask[n,c] * ( gamma * (x - mean) * invstd + beta ) )
 * `mask` (N*C floats, 0 or 1/(1-p)) may be NULL (no dropout).
 * save_mean / save_invstd (C floats each) are outputs in training mode and
 * inputs to the backward.  In eval mode (training = 0) running stats are used.
 */
size_t dcv_bn_workspace_bytes(int channels);
int dcv_bn_act_forward(const float* x, const dcv_dims5* xd, float* y, const dcv_dims5* yd,
                       const float* gamma, const float* beta,
                       float* running_mean, float* running_var, int64_t* num_batches_tracked /* may be NULL; += 1 when training */,
                       float* save_mean, float* save_invstd,
                       const float* mask, int training, float momentum, float eps,
                       int act, float slope, void* ws, size_t ws_bytes, void* stream);
/* dx, dgamma, dbeta from dy; x is the BN input, y unused. dgamma/dbeta are
 * OVERWRITTEN (C floats each). */
/* dcv_bn_act_forward with the batch statistics taken from dcv_conv_forward_stats' partial sums (training mode) */
int dcv_bn_act_forward_stats(const float* x, const dcv_dims5* xd, float* y, const dcv_dims5* yd, const float* gamma, const float* beta,
                             float* running_mean, float* running_var, int64_t* num_batches_tracked, float* save_mean, float* save_invstd, const float* mask,
                             float momentum, float eps, int act, float slope, const float* stat, int nparts, int pitch,
                             void* ws, size_t ws_bytes, void* stream);
int dcv_bn_act_backward(const float* dy, const dcv_dims5* dyd, const float* x, const dcv_dims5* xd,
                        float* dx, const dcv_dims5* dxd,
                        const float* gamma, const float* beta, const float* save_mean, const float* save_invstd,
                        const float* mask, int training, int act, float slope,
                        float* dgamma, float* dbeta, void* ws, size_t ws_bytes, void* stream);

/* ---- synchronised BatchNorm (data parallel; fp32 path; added symbols only: the ABI version stays 4) ----
 * Training-mode BatchNorm whose statistics and backward sums cover the batch of ALL ranks.  A "row" is 2*C + 1 doubles: {s0[c]}, {s1[c]}, count.
 * Each rank writes its own row, the caller exchanges them into the table rows = double[world][2*C + 1] in device memory (one collective per BatchNorm
 * group and pass, e.g. an all-reduce(SUM) of a zeroed table in which each rank filled its own row), and every rank then adds the same table in rank
 * order in fp64: identical bits on every rank.  Forward:  sync_sums -> exchange -> sync_finalize -> dcv_bn_apply.
 *                                              Backward: sync_backward_sums -> exchange -> sync_backward_apply.
 * ws: dcv_bn_workspace_bytes(C).  Checks as in the entries above: DCV_EINVAL, DCV_EWORKSPACE before any launch, DCV_EUNSUPPORTED beyond 2^32 groups.
 *  - sync_sums: sum x, sum x^2 and the element count of this rank's x.  stat == NULL: its own pass over x (the `split` partials of a channel are added in
 *    index order); otherwise the producing convolution's epilogue partials (dcv_conv_forward_stats), added as dcv_bn_act_forward_stats adds them (ws unused).
 *  - sync_finalize: per channel, the rows' sums and counts added in rank order, then save_mean / save_invstd, the running statistics (unbiased variance
 *    with the GLOBAL count; may both be NULL) and num_batches_tracked += 1 (may be NULL) exactly as dcv_bn_act_forward leaves them.
 *  - sync_backward_sums: sum dz, sum dz * xhat (dz = dy * act'(z) * mask) and the count of this rank.
 *  - sync_backward_apply: dgamma / dbeta = this rank's OWN sums rows[rank] (a gradient all-reduce adds the ranks later, as for every other parameter);
 *    dx = gamma * invstd * (dz - S0 / N - xhat * S1 / N) with S and N summed over all rows in rank order. */
size_t dcv_bn_sync_row_doubles(int channels);
int dcv_bn_sync_sums(const float* x, const dcv_dims5* xd, const float* stat, int nparts, int pitch, double* row, void* ws, size_t ws_bytes, void* stream);
int dcv_bn_sync_finalize(const double* rows, int world, int channels, float eps, float momentum, float* running_mean, float* running_var, int64_t* num_batches_tracked,
                         float* save_mean, float* save_invstd, void* stream);
int dcv_bn_sync_backward_sums(const float* dy, const dcv_dims5* dyd, const float* x, const dcv_dims5* xd, const float* gamma, const float* beta,
                              const float* save_mean, const float* save_invstd, const float* mask, int act, float slope, double* row,
                              void* ws, size_t ws_bytes, void* stream);
int dcv_bn_sync_backward_apply(const float* dy, const dcv_dims5* dyd, const float* x, const dcv_dims5* xd, float* dx, const dcv_dims5* dxd,
                               const float* gamma, const float* beta, const float* save_mean, const float* save_invstd, const float* mask, int act, float slope,
                               const double* rows, int world, int rank, float* dgamma, float* dbeta, void* ws, size_t ws_bytes, void* stream);

/* ---- elementwise --------------------------------------------------------- */
/* y = act(x)  /  dx = dy * act'(.) evaluated from the OUTPUT y
 * (nn.LeakyReLU generator.py:175, discriminator.py:84,90,186; nn.Tanh generator.py:78,276) */
int dcv_act_forward(const float* x, const dcv_dims5* xd, float* y, const dcv_dims5* yd, int act, float slope, void* stream);
int dcv_act_backward(const float* dy, const dcv_dims5* dyd, const float* y, const dcv_dims5* yd,
                     float* dx, const dcv_dims5* dxd, int act, float slope, void* stream);
/* y = a*x + b*z   (z may be NULL): Noise add with an injected sample
 * (discriminator.py:30-39), temporal difference of gdis (discriminator.py:330-331),
 * gradient accumulation, strided copies (torch.cat at generator.py:393-400,
 * discriminator.py:124,228 is two such copies into channel slices). */
int dcv_axpby(const float* x, const dcv_dims5* xd, float a, const float* z, const dcv_dims5* zd, float b,
              float* y, const dcv_dims5* yd, void* stream);
/* y = x + sigma * N(0,1) drawn on the device (Philox4x32-10 + Box-Muller), the
 * production form of discriminator.py:30-39.  (seed, offset) select the stream. */
int dcv_noise_add(const float* x, const dcv_dims5* xd, float* y, const dcv_dims5* yd,
                  float sigma, uint64_t seed, uint64_t offset, void* stream);
/* out[i] = N(0,1), i < n   (latents: generator.py:85,88,104,356) */
int dcv_normal_fill(float* out, int64_t n, uint64_t seed, uint64_t offset, void* stream);
/* `count` consecutive draws of n values each, out[j * n + i]: draw j holds exactly what dcv_normal_fill(.., seed, offset + j) would write (one launch for the
 * generator's per-frame motion noise, models.py / generator.py:57-62 of the reference: video_length draws of (batch, dim_z_motion)). */
int dcv_normal_fill_many(float* out, int64_t n, int64_t count, uint64_t seed, uint64_t offset, void* stream);
/* Dropout2d(p) plane mask: mask[i] = Bernoulli(1-p) / (1-p), i < n = N*C (generator.py:211,248) */
int dcv_dropout_mask(float* mask, int64_t n, float p, uint64_t seed, uint64_t offset, void* stream);

/* ---- input pipeline (dataset.py:125-186): disk-order frames -> training tensors ----------- *
 * out (B,C,T,H,W) fp32 = float(in (B,T,H,W,C)) / div - sub, numpy's fp32 operation order:
 * colour / depth PNG frames: in uint8, div 127.5, sub 1.0 (dataset.py:131, 168);
 * optical flow: in fp32, div image_size, sub 0 (dataset.py:174).                              */
int dcv_decode_video(const void* in, int in_is_u8, int B, int T, int H, int W, int C, float div, float sub, float* out, void* stream);
/* SURREAL depth (dataset.py:137-156): depth (B,T,H,W) fp32 with background >= 1e10 -> out (B,1,T,H,W):
 * foreground min-max normalised per clip to [-1, 0.8], background 1.0; ws_minmax: 2*B floats.  */
int dcv_surreal_depth(const float* depth, int B, int T, int H, int W, float* out, float* ws_minmax, void* stream);

/* ---- segmentation branch (surreal-segm.yml, 25 body-part channels) ---------- *
 * softmax over the channel axis = the geometry generator's nn.Softmax(dim=1) head (generator.py:75-76)  */
int dcv_softmax_channels_forward(const float* x, const dcv_dims5* xd, float* y, const dcv_dims5* yd, void* stream);
int dcv_softmax_channels_backward(const float* dy, const dcv_dims5* dyd, const float* y, const dcv_dims5* yd, float* dx, const dcv_dims5* dxd, void* stream);
/* one-hot / softmax maps -> {-1,+1} maps: argmax over channels (first maximum), scatter (generator.py:378-385) */
int dcv_segm_onehot(const float* x, const dcv_dims5* xd, float* y, const dcv_dims5* yd, void* stream);
/* argmax -> part colour (util.py:236-246); palette = C x 3 bytes on the device; out uint8 (N,3,D,H,W)  */
int dcv_segm_to_rgb(const float* x, const dcv_dims5* xd, const uint8_t* palette, uint8_t* out, void* stream);
/* dataset.py:176-181: label frames uint8 (B,T,H,W) -> one-hot fp32 (B,C,T,H,W)                       */
int dcv_decode_segmentation(const uint8_t* labels, int B, int T, int H, int W, int C, float* out, void* stream);

/* ---- sampling path: float videos -> uint8 on the device --------------------- *
 * util.videos_to_numpy (util.py:58-79) and the depth branch of
 * util.geometric_info_in_color_format (util.py:219-222): out = uint8((clip(x,-1,1)+1)/2*255),
 * same fp32 operation order (bytes identical); out is contiguous (N, C*channel_repeat, D, H, W).  */
int dcv_videos_to_uint8(const float* x, const dcv_dims5* xd, uint8_t* out, int channel_repeat, void* stream);
/* util.visualize_optical_flow (util.py:143-170) for a (B,2,T,H,W) flow video scaled by `scale`
 * (= H, util.py:227): hue = direction, value = per-frame min-max normalised magnitude; out uint8
 * (B,3,T,H,W); ws_minmax: 2*B*T floats of scratch. */
int dcv_flow_to_rgb(const float* flow, const dcv_dims5* fd, float scale, uint8_t* out, float* ws_minmax, void* stream);

/* ---- GAN losses (fused value + gradient) --------------------------------- *
 * loss.py:91-99,123-131 (BCE-with-logits, sum / numel) and loss.py:163-164,
 * 190-191 (hinge / softplus).  kind: 0 = BCE target 1, 1 = BCE target 0,
 * 2 = mean(relu(1 - y)), 3 = mean(relu(1 + y)), 4 = mean(softplus(-y)).
 * *loss_out (+)= value ; dy_out[i] = d value / d y[i].                        */
int dcv_gan_loss(const float* y, int64_t n, int kind, float* loss_out, int accumulate, float* dy_out, void* stream);
/* y[i] = x[i] * *s, s a 0-d DEVICE scalar: the backward of a loss term — `loss.backward()` (trainer.py:319,356) hands every
 * term of loss.py:99,131,164,191 the upstream cotangent as a device tensor; dy_out of dcv_gan_loss times it, without a host read. */
int dcv_scale_dev(const float* x, int64_t n, const float* s, float* y, void* stream);

/* ---- GRUCell (generator.py:58,94) --------------------------------------- *
 * The whole T-step motion-latent recurrence in one launch: h_t = GRU(e_t, h_{t-1}).
 * e: (T, B, dm) noise, h0: (B, dm); out: (B, T, dm) (= torch.stack(h[1:], 1));
 * gates: (T, B, 4*dm) saved [r, z, n, hn_pre] for the backward.                */
size_t dcv_gru_workspace_bytes(int B, int dm);
int dcv_gru_forward(const float* e, const float* h0, const float* w_ih, const float* w_hh,
                    const float* b_ih, const float* b_hh, float* out, float* gates,
                    int T, int B, int dm, void* stream);
int dcv_gru_backward(const float* dout, const float* e, const float* h0, const float* out, const float* gates,
                     const float* w_ih, const float* w_hh,
                     float* dw_ih, float* dw_hh, float* db_ih, float* db_hh,
                     int T, int B, int dm, void* ws, size_t ws_bytes, void* stream);

/* ---- Adam (train.py:171-176: betas (0.5, 0.999), eps 1e-8, L2 weight decay) */
/* torch.optim.Adam's update operation for operation; the bias corrections 1 - beta^step and the step size
 * lr / (1 - beta1^step) are formed in double on the host (torch forms them as Python floats) and rounded once.
 * g is scaled by grad_scale first (1 / world size under data parallelism, 1 otherwise). */
int dcv_adam_step(float* p, const float* g, float* m, float* v, int64_t n,
                  double lr, double beta1, double beta2, double eps, double weight_decay, int step,
                  double grad_scale, void* stream);
/* the same update for n_tensors parameter tensors of one optimiser (one shared step count) in ceil(n/24) launches */
int dcv_adam_step_multi(int n_tensors, float* const* p, const float* const* g, float* const* m, float* const* v, const int64_t* numel,
                        double lr, double beta1, double beta2, double eps, double weight_decay, int step, double grad_scale, void* stream);

/* ---- gradient guard: global norm, clipping, non-finite skip, loss scale — decided on the device ------ *
 * `state` is DCV_GUARD_STATE_FLOATS floats in device memory, owned by the caller, who initialises it once
 * (loss scale, everything else 0) and afterwards only reads it:                                            */
#define DCV_GUARD_LOSS_SCALE 0     /* the scale the NEXT backward multiplies the loss by (its root cotangent)          */
#define DCV_GUARD_GROWTH_TRACKER 1 /* finite measurements since the scale last changed (dynamic scaling)              */
#define DCV_GUARD_GRAD_NORM 2      /* L2 norm of the TRUE gradients: sqrt(sum g^2) * grad_scale / (scale of the measured backward) */
#define DCV_GUARD_CLIP_COEF 3      /* min(1, max_norm / (norm + 1e-6)); 1 without clipping or on a non-finite measurement */
#define DCV_GUARD_FACTOR 4         /* grad_scale * clip_coef / scale: what the guarded Adam multiplies g by (before weight decay) */
#define DCV_GUARD_SKIPPED 5        /* 1 if the steps on this measurement are skipped, else 0                          */
#define DCV_GUARD_SKIPPED_TOTAL 6  /* measurements that ended in a skip so far                                        */
#define DCV_GUARD_NONFINITE 7      /* inf / NaN elements in the last measurement                                      */
#define DCV_GUARD_STATE_FLOATS 8
/* bytes of `ws` for a measurement over n_tensors tensors of total_elements elements in all (0 + DCV_EINVAL text for negative arguments) */
size_t dcv_grad_guard_workspace_bytes(int64_t total_elements, int n_tensors);
/* One measurement, ceil(n_tensors / 24) + 1 launches, no atomics (bitwise repeatable): per-block partial sums of squares (fp32 within a thread's 16 elements,
 * double above) and counts of elements whose exponent bits are all ones, then one workgroup that adds them in a fixed order and writes GRAD_NORM .. NONFINITE.
 * The measurement is NON-FINITE if any element is, or if the sum of squares is not finite (finite elements whose squares overflow fp32 count as non-finite);
 * it is SKIPPED if it is non-finite and skip_nonfinite is set.  max_norm <= 0: no clipping.  `dynamic` then updates the loss scale as torch.amp.GradScaler does:
 * non-finite: scale *= backoff_factor, tracker = 0; else tracker += 1 and, when it reaches growth_interval, scale *= growth_factor, tracker = 0.  FACTOR uses
 * the scale as it was BEFORE this update, i.e. the one the measured backward ran with.  Call it once per backward. */
int dcv_grad_guard_measure(int n_tensors, const float* const* g, const int64_t* numel, double grad_scale, double max_norm, int skip_nonfinite, int dynamic,
                           double growth_factor, double backoff_factor, int growth_interval, float* state, void* ws, size_t ws_bytes, void* stream);
/* dcv_adam_step_multi with the step count and the decision on the device.  `step_block` is DCV_ADAM_STEP_BLOCK_BYTES of device memory, zeroed by the caller before
 * the first step and shared by tensors with one step count: step_block[0] is that count; the rest is scratch of the call (skip flag, the update's scalars).
 * A one-thread kernel reads state[DCV_GUARD_SKIPPED]; unless set it increments step_block[0] and forms the bias corrections from it in double, with
 * state[DCV_GUARD_FACTOR] in grad_scale's place; the update kernels (unchanged arithmetic) read them.  A skipped step touches no p, m, v and no step count.
 * 1 + ceil(n_tensors / 24) launches. */
#define DCV_ADAM_STEP_BLOCK_BYTES 64
int dcv_adam_step_multi_guarded(int n_tensors, float* const* p, const float* const* g, float* const* m, float* const* v, const int64_t* numel,
                                double lr, double beta1, double beta2, double eps, double weight_decay, int32_t* step_block, const float* state, void* stream);

/* ---- EMA of model weights (the twin a GAN is sampled from): count, warm-up and skip decided on the device ------ *
 * One update of n_tensors tensors: ema[t] += w (src[t] - ema[t]) as ONE fmaf(w, src - ema, ema) per element, with w = (float)(1 - d),
 * d = warmup ? min(decay, (1 + t) / (10 + t)) : decay in double, t = the number of updates applied so far.  `ema_block` is DCV_EMA_BLOCK_BYTES of device memory,
 * zeroed by the caller once: ema_block[0] is that number (a host may read it back); the rest is scratch of the call (skip flag, w).
 * A one-thread kernel reads guard_state[DCV_GUARD_SKIPPED] (NULL: never skipped); unless set it forms w and increments ema_block[0]; the update kernels read them.
 * A skipped update touches no ema tensor and no count.  16-byte loads and stores where both bases of a tensor are 16-byte aligned, single elements otherwise.
 * No atomics (bitwise repeatable).  decay in [0, 1); numel 0 is allowed (nothing is launched for it, its pointers are not looked at).  1 + ceil(n_tensors / 24) launches. */
#define DCV_EMA_BLOCK_BYTES 64
/* mode[t]: 0 = average (fp32), 1 = copy dwords (buffers; an int64 tensor is passed as 2 * numel dwords) */
int dcv_ema_update_multi(int n_tensors, float* const* ema, const float* const* src, const int64_t* numel, const int32_t* mode,
                         double decay, int warmup, int32_t* ema_block, const float* guard_state /* may be NULL */, void* stream);

/* ---- spectral normalisation of convolution weights (the discriminators' Lipschitz control), fp32 ------ *
 * A weight is a contiguous matrix W of rows[t] rows (cout) and cols[t] columns (cin * kd * kh * kw).  One update with n_iter power iterations:
 *   repeat n_iter:  t = W^T u ; v = t / max(|t|, eps) ; s = W v ; u = s / max(|s|, eps)
 *   sigma = u^T (W v)   (n_iter = 0: of the stored u, v) ;  w_sn = W / max(sigma, eps)        (a zero matrix gives w_sn = 0, not NaN)
 * Products and a thread's running sums are fp32; block partials are double and are added in a fixed order; the norms, 1 / norm and 1 / sigma are formed by one thread
 * in double (sqrt and one division) and rounded to fp32 once.  No atomics: the same inputs give the same bits.  16-byte loads where a tensor's base (and, for the
 * matrix passes, its row pitch) allow, single elements otherwise; pointers need 4-byte alignment only.  `w` is never written.
 * LAUNCHES, a function of n_tensors, n_iter and the guard only: ceil(n_tensors / 24) * (n_iter > 0 ? 2 * n_iter + 1 : 2) + (guard_state ? 1 : 0) for an update,
 * 2 * ceil(n_tensors / 24) for a projection.
 * With guard_state a one-thread kernel reads guard_state[DCV_GUARD_SKIPPED] first; a skipped update writes no u, v, sigma or w_sn.
 * `ws`: dcv_spectral_workspace_bytes(n, rows, cols) bytes of device memory on a 16-byte boundary, scratch of one call (update or projection).
 * rows, cols >= 1 and rows * cols <= 2^30. */
size_t dcv_spectral_workspace_bytes(int n_tensors, const int32_t* rows, const int32_t* cols);
int dcv_spectral_update_multi(int n_tensors, const float* const* w, float* const* w_sn, float* const* u, float* const* v, float* const* sigma,
                              const int32_t* rows, const int32_t* cols, int n_iter, double eps, const float* guard_state /* may be NULL */,
                              void* ws, size_t ws_bytes, void* stream);
/* The gradient with respect to W of a loss whose gradient with respect to w_sn is g, with u and v held constant, in place on g:
 *   g <- (g - <g, w_sn> u v^T) / max(sigma, eps)        (eps: the update's, so that both divide by the same number)
 * It is linear in g: apply it once to the SUM of the gradients of all uses of one (w_sn, u, v, sigma).  w_sn, u, v and sigma are not written. */
int dcv_spectral_project_multi(int n_tensors, float* const* g, const float* const* w_sn, const float* const* u, const float* const* v, const float* const* sigma,
                               const int32_t* rows, const int32_t* cols, double eps, void* ws, size_t ws_bytes, void* stream);

/* ---- adaptive clip augmentation in front of the discriminators (DiffAugment's transforms, ADA's probability), fp32 ------ *
 * The reference shows the discriminators the clips as they are (trainer.py:299-309 the real pair and the D phase's fakes, trainer.py:344-349 the G phase's fakes);
 * these entries transform a clip pair between those lines and the discriminators' forward, differentiably (added symbols only: the ABI version stays 4).
 * One row of `table` = int32[table_rows][8] per clip serves all frames and both streams of a pair:                                                          */
#define DCV_AUG_T_FLIP 0       /* 0 or 1: mirror left-right                                                                    */
#define DCV_AUG_T_DX 1         /* shift right by dx pixels, zero padding                                                       */
#define DCV_AUG_T_DY 2         /* shift down by dy pixels                                                                      */
#define DCV_AUG_T_CUT_Y0 3     /* the cutout box [cut_y0, cut_y0 + cut_size) x [cut_x0, cut_x0 + cut_size); may hang over a border */
#define DCV_AUG_T_CUT_X0 4
#define DCV_AUG_T_CUT_SIZE 5   /* 0: no cutout                                                                                 */
#define DCV_AUG_T_GAIN 6       /* fp32 bits                                                                                    */
#define DCV_AUG_T_BIAS 7       /* fp32 bits.  The identity row is {0, 0, 0, 0, 0, 0, bits(1.0f), bits(0.0f)}                   */
/* y[b, c, t, h, w] = 0 inside the cutout box; else with hs = h - dy, ws = w - dx: 0 if (hs, ws) is outside the plane (padding is zero AFTER the colour step); else
 *   v = x[b, c, t, hs, flip ? W - 1 - ws : ws],  y = sgn * v * gain + bias  as two separately rounded fp32 operations (never one fma).
 * `colour` = 0 (the geometry stream): gain 1, bias 0 and NO arithmetic: the bits are moved (-0.0 and NaN payloads survive).  sgn = -1 where flip is set and
 * c == flip_negate_channel (-1: no such channel; 0 for an optical-flow clip, whose horizontal component changes sign under a mirror, util.py:160), exact.
 * x: any strided view; y: contiguous (N, C, D, H, W).  16-byte stores where y's base allows (W % 4 == 0), 16-byte loads where dx % 4 == 0, there is no flip and
 * x's base and pitches allow, dword loads otherwise; W % 4 != 0 or a w stride other than 1 takes one element per lane.  One launch.
 * (The adjoint's output dx may be any strided view: a gradient is best written in the layout of the tensor it belongs to.)
 * dcv_aug_apply_backward is the adjoint, also a gather (no atomics): for source pixel (hs, wsrc), ws = flip ? W - 1 - wsrc : wsrc, (h, w) = (hs + dy, ws + dx);
 *   dx_out = (sgn * gain) * dy_in[h, w] (one rounding; gain 1 on the geometry stream) if (h, w) is inside the plane and outside the box, else 0.  bias has no gradient.
 * DCV_EINVAL before any launch: shapes that differ, table_rows != N, an output that is not contiguous; DCV_EUNSUPPORTED: H or W above 4096. */
int dcv_aug_apply(const float* x, const dcv_dims5* xd, const int32_t* table, int table_rows, float* y, const dcv_dims5* yd, int colour, int flip_negate_channel,
                  void* stream);
int dcv_aug_apply_backward(const float* dy, const dcv_dims5* dyd, const int32_t* table, int table_rows, float* dx, const dcv_dims5* dxd, int colour,
                           int flip_negate_channel, void* stream);
/* The adjoint for a clip that several consumers read (the fakes' geometry clip: the colour generator reads it as it is, two discriminators read the augmented clip
 * and the image discriminator reads frame `frame` of it, trainer.py:303-309,344-349), as ONE gather that also forms the sum, in the operands' order:
 *   dx = ((base + A^T dy0) + A^T dy1) + A^T embed(dyf)      with A^T = dcv_aug_apply_backward and embed() placing the (N, C, 1, H, W) cotangent at frame `frame`.
 * base (already in the clip's own space), dy1 and dyf may be NULL (with their dims), not all of dy0, dy1, dyf.  With the identity row every A^T moves bits, so the sum
 * is the one the un-augmented fan-in forms, addition for addition.  dx: any strided view (e.g. the clip's own layout), as for dcv_aug_apply_backward. */
int dcv_aug_fan_backward(const float* base, const dcv_dims5* based, const float* dy0, const dcv_dims5* dy0d, const float* dy1, const dcv_dims5* dy1d,
                         const float* dyf, const dcv_dims5* dyfd, int frame, const int32_t* table, int table_rows, float* dx, const dcv_dims5* dxd, int colour,
                         int flip_negate_channel, void* stream);
/* The state block: DCV_AUG_STATE_WORDS 32-bit words in device memory, owned by the caller, who initialises it once (p, everything else 0). */
#define DCV_AUG_P 0            /* fp32 bits: the probability of each enabled transform                                          */
#define DCV_AUG_SUM_SIGN 1     /* int32: sum of sign(D(real)) since the last adjustment                                        */
#define DCV_AUG_COUNT 2        /* int32: logits observed since the last adjustment                                             */
#define DCV_AUG_ADJUSTS 3      /* int32: adjustments made                                                                      */
#define DCV_AUG_STATE_WORDS 8  /* words 4-7 reserved, zero                                                                     */
#define DCV_AUG_FLIP 1
#define DCV_AUG_TRANSLATE 2
#define DCV_AUG_CUTOUT 4
#define DCV_AUG_COLOUR 8
typedef struct dcv_aug_limits {      /* a host struct, passed by value to the kernel */
    int32_t mx, my;                  /* |dx| <= mx, |dy| <= my                                           */
    int32_t size;                    /* side of the cutout box                                           */
    int32_t mask;                    /* DCV_AUG_FLIP | _TRANSLATE | _CUTOUT | _COLOUR: the enabled ops   */
    float contrast, brightness;      /* gain in 1 + 2 contrast (u - 0.5), bias in brightness (u - 0.5)   */
} dcv_aug_limits;
/* One thread per clip draws its row: Philox4x32-10 with key = seed, counter = {idx lo, idx hi, offset lo, offset hi}, block j of clip b at idx = 4 b + j, words
 * w0..w3 of a block; u(r) = ((float)r + 0.5f) * 2^-32 in (0, 1].  p = state[DCV_AUG_P], read on the device.  A gate is on <=> its op is enabled and u <= p.
 *   block 0: w0 flip gate; flip = gate && (w1 >> 31); w2 translate gate          block 1: dx = (int)(w0 % (2 mx + 1)) - mx; dy likewise from w1, my; w2 cutout gate
 *   block 2: cut_y0 = (int)(w0 % H) - size / 2; cut_x0 = (int)(w1 % W) - size / 2; w2 colour gate
 *   block 3: gain = 1 + (2 contrast) * (u(w0) - 0.5), bias = brightness * (u(w1) - 0.5), every operation rounded to fp32 on its own.
 * A gate that is off writes its op's identity words: p = 0 gives identity rows, p = 1 turns every enabled gate on. */
int dcv_aug_draw(int32_t* table, int B, int H, int W, const int32_t* state, const dcv_aug_limits* limits, uint64_t seed, uint64_t offset, void* stream);
/* ---- interpolated warps and saturation: the (N, 24) row (added symbols only: the ABI version stays 4; dcv_aug_limits is unchanged) ------ *
 * Words 0-7 are the row above.  Word 8 `warp`: 0 = the exact integer path of words 0-2 (bits moved), non-zero = interpolating, where words 9-18 govern the geometry
 * and words 0-2 are already composed into them.  Words 9-14: a b c d e f (fp32 bits), the inverse map in centred pixel coordinates.  Words 15-18: l00 l01 l10 l11,
 * the forward linear part L = inverse of [[a, b], [d, e]], written by the draw and never inverted in a kernel.  Word 19: saturation s (1.0 = identity, and exactly
 * 1.0 skips the step).  Words 20-23 reserved, zero.  Identity extension: {0, 1,0,0, 0,1,0, 1,0,0,1, 1.0, 0,0,0,0}.
 * Every operation is ONE separately rounded fp32 operation; a unary minus below is 0 - x.  The numpy restatement is tests/augwarp.py.
 * Forward, warp != 0, output pixel (h, w): 0 inside the cutout box; else cx = (W-1)*0.5, cy = (H-1)*0.5, u = w - cx, v = h - cy, su = (a*u + b*v) + c,
 *   sv = (d*u + e*v) + f, sx = su + cx, sy = sv + cy, x0 = floor(sx), fx = sx - x0 (y alike); non-finite sx or sy gives 0; indices are clamped to [-2, W] before the
 *   float-to-int conversion.  Taps (y0,x0) (y0,x0+1) (y0+1,x0) (y0+1,x0+1) with weights (1-fy)(1-fx), (1-fy)fx, fy(1-fx), fy fx; a tap outside the plane or of weight
 *   exactly 0 is skipped; acc = +0, acc = acc + weight * value in tap order.  Colour stream: value = the colour step on the tap's source pixel,
 *   m = ((v0+v1)+v2) * third (third = 0x3EAAAAAB), q_c = m + s*(v_c - m) (only when C == 3 and s != 1), y_c = q_c*gain + bias.  vector_channels = 1 (optical flow, C >= 2):
 *   (r0', r1') = (l00*r0 + l01*r1, l10*r0 + l11*r1) after sampling.  warp == 0: dcv_aug_apply's bits, vector_channels = 1 meaning flip_negate_channel = 0; with
 *   s != 1 the colour step above on the one source pixel.  colour and vector_channels are not both set, and vector_channels = 1 needs C >= 2 (DCV_EINVAL).
 * Adjoint, warp != 0, a gather over source pixels p = (ys, xs): du = (xs - cx) - c, dv = (ys - cy) - f, centre ocx = (l00*du + l01*dv) + cx, ocy = (l10*du + l11*dv) + cy,
 *   half-extents ex = min((|l00| + |l01|) + 1, 4), ey alike; candidates h in [max(ceil(ocy - ey), 0), min(floor(ocy + ey), H-1)] ascending, then w alike: at most 9 x 9.
 *   A candidate outside the box whose recomputed taps (the forward's operations) contain p with a non-zero weight is a hit.  The hit list has room for 25, the lattice-point bound
 *   A + P/2 + 1 of the rectangle L (-1, 1)^2 under dcv_aug_warp_draw's limits (sx, sy <= 2), so no drawn row loses a hit; a hand-made row is in contract when
 *   4 |det L| + 2 (|L e1| + |L e2|) + 1 <= 25 (beyond that the first 25 in scan order count);
 *   acc = +0, acc = acc + weight * t, t the cotangent there, on vector channels first mixed by L^T: t0 = l00*d0 + l10*d1, t1 = l01*d0 + l11*d1.  Colour stream, on
 *   the gathered t_c: a_c = gain*t_c, ma = ((a0+a1)+a2)*third, dv_c = ma + s*(a_c - ma).  warp == 0: dcv_aug_apply_backward's bits.  An L outside the box cap is out
 *   of contract: memory-safe, adjoint unspecified; dcv_aug_warp_draw never makes one.
 * The fan-in entry forms ((base + A^T dy0) + A^T dy1) + A^T embed(dyf), each A^T term complete before it is added.  One launch each; no atomics.  Any table is memory-safe. */
#define DCV_AUG_WARP_ROW_WORDS 24
#define DCV_AUG_T_WARP 8
#define DCV_AUG_T_INV 9        /* a b c d e f                                                                                  */
#define DCV_AUG_T_FWD 15       /* l00 l01 l10 l11                                                                              */
#define DCV_AUG_T_SAT 19
int dcv_aug_warp_apply(const float* x, const dcv_dims5* xd, const int32_t* table, int table_rows, float* y, const dcv_dims5* yd, int colour, int vector_channels,
                       void* stream);
int dcv_aug_warp_apply_backward(const float* dy, const dcv_dims5* dyd, const int32_t* table, int table_rows, float* dx, const dcv_dims5* dxd, int colour,
                                int vector_channels, void* stream);
int dcv_aug_warp_fan_backward(const float* base, const dcv_dims5* based, const float* dy0, const dcv_dims5* dy0d, const float* dy1, const dcv_dims5* dy1d,
                              const float* dyf, const dcv_dims5* dyfd, int frame, const int32_t* table, int table_rows, float* dx, const dcv_dims5* dxd, int colour,
                              int vector_channels, void* stream);
#define DCV_AUG_SCALE 16
#define DCV_AUG_ROTATE 32
#define DCV_AUG_ANISO 64
#define DCV_AUG_SUBPIXEL 128
#define DCV_AUG_SATURATION 256
typedef struct dcv_aug_warp_limits {      /* a host struct, passed by value to the kernel */
    float scale_max, aniso_max;      /* >= 1, scale_max * aniso_max <= 2: every drawn L stays inside the adjoint's box               */
    float rot_tan_half;              /* tan(rot_max / 2), computed once on the host                                                 */
    float frac;                      /* sub-pixel shift up to frac * W, frac * H                                                     */
    float sat;                       /* s in 1 + sat * (-1, 1]                                                                       */
    int32_t mask;                    /* DCV_AUG_SCALE | _ROTATE | _ANISO | _SUBPIXEL | _SATURATION                                   */
} dcv_aug_warp_limits;
/* Words 0-7 are what dcv_aug_draw writes for the same (seed, offset, p) (blocks 0-3 at idx = 4 b + j).  Extension blocks j = 4..6 of clip b at idx = 4 B + 4 b + (j - 4);
 * vv(u) = (u + u) - 1; ratio(u, m): k = (m - 1) * |vv|, vv >= 0 ? 1 + k : 1 / (1 + k).  + - * / only, each rounded on its own.
 *   block 4: w0 scale gate; w1 s_iso = ratio(u, scale_max); w2 rotate gate; w3 t = rot_tan_half * vv, den = 1 + t*t, cos = (1 - t*t) / den, sin = (t + t) / den
 *            (the angle is 2 atan(t): slightly non-uniform in theta, denser towards 0)
 *   block 5: w0 aniso gate; w1 r = ratio(u, aniso_max), sx = s_iso * r, sy = s_iso / r; w2 sub-pixel gate; w3 tx = (frac * W) * vv
 *   block 6: w0 ty = (frac * H) * vv; w1 saturation gate; w2 s = 1 + sat * vv.        A gate that is off writes its identity.
 * phi = flip ? -1 : 1, tau = (dx + tx, dy + ty); p_out = R diag(sx, sy) diag(phi, 1) p_src + tau:
 *   l00 = (cos*sx)*phi, l01 = 0 - sin*sy, l10 = (sin*sx)*phi, l11 = cos*sy; a = phi*(cos/sx), b = phi*(sin/sx), d = 0 - sin/sy, e = cos/sy;
 *   c = 0 - (a*taux + b*tauy), f = 0 - (d*taux + e*tauy).  warp = 1 iff a scale, rotate, aniso or sub-pixel gate is on; words 9-18 are written either way. */
int dcv_aug_warp_draw(int32_t* table, int B, int H, int W, const int32_t* state, const dcv_aug_limits* limits, const dcv_aug_warp_limits* warp_limits, uint64_t seed,
                      uint64_t offset, void* stream);
/* state[SUM_SIGN] += sum sign(logits[i]) (sign(0) = 0, a NaN counts 0), state[COUNT] += n. One workgroup, integer sums: exact and repeatable.  1 <= n <= 2^24. */
int dcv_aug_observe(const float* logits, int64_t n, int32_t* state, void* stream);
/* ADA's rule (Karras et al. 2020) with r = E[sign(D(real))], one thread: if COUNT > 0: r = SUM_SIGN / COUNT in double, p = min(max(p + sgn(r - target) * step, 0), p_max)
 * in fp32 (sgn(0) = 0).  Then SUM_SIGN = COUNT = 0 and ADJUSTS += 1.  The host calls it every `interval` iterations; nothing is read back. */
int dcv_aug_adjust(int32_t* state, double target, float step, float p_max, void* stream);

/* ---- LeCam regularisation of the discriminators (Tseng et al. 2021), anchors kept on the device, fp32 ------ *
 * The reference's discriminator losses are loss.py:91-99,163-164 alone; these entries add weight * (mean(relu(D(real) - aF)^2) + mean(relu(aR - D(fake))^2)) to the
 * value and the stored gradient dcv_gan_loss left, with the anchors aR / aF = an EMA of each discriminator's mean logit on the real / fake batch
 * (added symbols only: the ABI version stays 4).  Tables (y_real[], y_fake[], n_real[], n_fake[], loss[], dy_real[], dy_fake[]) are HOST arrays of n_dis entries.
 * The state: n_dis blocks of DCV_LECAM_STATE_WORDS 32-bit words in device memory, owned by the caller, who zeroes it once.                                 */
#define DCV_LECAM_ANCHOR_REAL 0   /* fp32 bits: EMA of mean D(real)                                                               */
#define DCV_LECAM_ANCHOR_FAKE 1   /* fp32 bits: EMA of mean D(fake)                                                               */
#define DCV_LECAM_UPDATES 2       /* int32: anchor updates applied so far                                                         */
#define DCV_LECAM_ACTIVE 3        /* int32: 1 if the last apply added the regulariser                                             */
#define DCV_LECAM_STATE_WORDS 8   /* words 4-7 reserved, zero                                                                     */
/* sums[k] = {sum y_real[k], (double)n_real[k], sum y_fake[k], (double)n_fake[k]} (sums: n_dis x 4 doubles in device memory).  THE SUM ORDER, here and for S_d, S_e
 * below: 256 lanes; lane l adds elements l, l + 256, ... in increasing index, each converted to double first, into a double that starts at +0.0; then for
 * s = 128, 64, .., 1 every lane l < s does p[l] += p[l + s]; the result is p[0].  One launch (one workgroup per discriminator), no atomics: the same input gives the
 * same bits.  Sums are additive over ranks: a data-parallel caller all-reduces `sums` (SUM) between the two entries. */
int dcv_lecam_sums(int n_dis, const float* const* y_real, const float* const* y_fake, const int64_t* n_real, const int64_t* n_fake, double* sums, void* stream);
/* For each discriminator k, with aR, aF, U = the state's anchors and UPDATES as they are BEFORE this call (the anchors are constants: no gradient flows through them):
 *   1. active = (U >= max(start, 1)); state[ACTIVE] = active.
 *   2. d_i = y_real[i] - aF, e_i = aR - y_fake[i], one fp32 subtraction each; one_sided: d_i = (d_i < 0 ? 0 : d_i), e_i likewise (a NaN stays a NaN).
 *      R = S_d / n_real + S_e / n_fake in double, S_d = sum (double)d_i * (double)d_i and S_e likewise, in the order above; r = (float)(weight * R), rounded once.
 *      active:     *loss[k] += r (one fp32 add); dy_real[k][i] += c_r * d_i; dy_fake[k][i] -= c_f * e_i with c_r = (float)(2 * weight / n_real), c_f likewise; product
 *                  and sum are rounded on their own (never one fma); reg[k] = r.
 *      not active: no byte of loss[k], dy_real[k], dy_fake[k] is written; reg[k] = 0.
 *   3. m_r = sums[k][0] / sums[k][1], m_f = sums[k][2] / sums[k][3] in double.  Either non-finite: the anchors and UPDATES stay as they are.  Else U == 0:
 *      aR = (float)m_r, aF = (float)m_f; otherwise aR = (float)((double)aR * decay + m_r * (1 - decay)), rounded once, aF likewise.  Then UPDATES += 1.
 * loss[k]: one 0-d device float; dy_*[k]: n_*[k] floats, read and modified.  One launch.  DCV_EINVAL before any launch unless 1 <= n_dis <= 8, 1 <= n <= 2^24 per
 * tensor, decay in [0, 1], weight finite and >= 0, no pointer NULL. */
int dcv_lecam_apply(int n_dis, const float* const* y_real, const float* const* y_fake, const int64_t* n_real, const int64_t* n_fake, const double* sums,
                    int32_t* state, double decay, int start, double weight, int one_sided, float* const* loss, float* const* dy_real, float* const* dy_fake,
                    float* reg, void* stream);

/* ---- the device-resident dataset: clips sampled and decoded on the device (added symbols only: the ABI version stays 4) ------ *
 * A stream's store is ONE packed buffer: the frames of all N videos back to back in disk order, video i at frames starts[i] .. starts[i+1] - 1 (`starts`: N + 1
 * int64 in device memory, a prefix sum of the frame counts of list.txt, dataset.py:86-97).  A batch is a (B, 2) int32 device table of rows (clip, t0): the clip is
 * frames t0 .. t0 + T - 1 of video `clip`.
 *
 * dcv_clipstore_draw replaces the DataLoader's shuffle (train.py:101-109: shuffle=True, drop_last=True; trainer.py:271) and the window draw of
 * dataset.py:116-123.  Row b is epoch position p = first_position + b (0 <= first_position, first_position + B <= N):
 *   clip = perm(p): a balanced Feistel network of 8 rounds on w = 2 h bits, w the smallest even width with 2^w >= N (at least 2), applied again while the value
 *          is >= N (cycle walking).  Round r: (L, R) <- (R, L ^ F_r(R)), starting from L = x >> h, R = x & (2^h - 1) and ending at x = L << h | R;
 *          F_r(R) = word 0 of Philox4x32-10(counter {R, r, epoch lo, epoch hi}, key {seed lo, seed hi}) & (2^h - 1).
 *   n = starts[clip + 1] - starts[clip];  t0 = 0 if n <= T, else mulhi32(u, n - T) in [0, n - T - 1] (np.random.randint(n - T), dataset.py:122: the last window
 *          is never drawn), u = word 0 of Philox4x32-10(counter {p, 0xFFFFFFFF, epoch lo, epoch hi}, same key).
 * One launch, one thread per row, no state: any position of any epoch is computed on its own.  1 <= N < 2^31. */
int dcv_clipstore_draw(int32_t* table, int B, const int64_t* starts, int64_t N, int T, uint64_t seed, uint64_t epoch, int64_t first_position, void* stream);
#define DCV_CLIP_U8 0       /* frames uint8 (F, H, W, C), 1 <= C <= 4: out = (float)x / div - sub   (colour, grey depth: div 127.5, sub 1; dataset.py:127-131, 158-166) */
#define DCV_CLIP_F32 1      /* frames fp32 (F, H, W, C), 1 <= C <= 4: out = x / div - sub           (optical flow: div image_size, sub 0; dataset.py:168-174)        */
#define DCV_CLIP_LABELS 2   /* frames uint8 (F, H, W): out = one-hot with C parts, C <= 256; div and sub unused (dataset.py:176-181)                                  */
/* out (B, C, T, H, W) fp32 contiguous = the table's windows of `frames`, normalised with the expressions of dcv_decode_video / dcv_decode_segmentation (one
 * definition, dcv_common.h): the bytes dataprep.decode_* writes for the same frames.  One launch.  All frame addressing is 64-bit; 16-byte loads where the window's
 * ADDRESS allows, 4-byte or single-byte loads otherwise.  A row that does not name T frames of one video (never drawn; the Python layer refuses it) is written as
 * NaN (one-hot: zeros) and nothing is read for it.  1 <= B <= 65535. */
int dcv_clipstore_gather(const void* frames, int mode, const int32_t* table, const int64_t* starts, int64_t N, int B, int T, int H, int W, int C, float div, float sub,
                         float* out, void* stream);
/* SURREAL depth (dataset.py:134-156), in place on `clips` = B gathered raw windows of per_clip fp32 metres each (DCV_CLIP_F32, C 1, div 1, sub 0): the foreground
 * (< 1e10) min-max of the WINDOW goes to [-1, 0.8], background 1.0 — dcv_surreal_depth's arithmetic.  One launch, one workgroup per clip. */
int dcv_clipstore_surreal(float* clips, int B, int64_t per_clip, void* stream);

/* ---- nearest-training-clip search on the device-resident dataset (added symbols only: the ABI version stays 4) ------ *
 * "Are the samples copies of training clips?"  The reference has no counterpart: it never compares a sample with the training set.  The store is a packed uint8
 * stream as above, frames of K = H*W*C bytes in disk order (H, W, C); a query clip is T frames of K bytes in the same order.  For a window (v, s), 0 <= s <= n_v - T:
 *   d(q, v, s) = sum_{t < T} sum_{j < K} ((int)q[t][j] - (int)frame[starts[v] + s + t][j])^2                                  (int64, exact)
 * and a query's result is the k windows with the smallest (d, v, s) in lexicographic order, except those of video exclude[q] (if >= 0); windows never cross a video
 * boundary; places beyond the admissible windows hold rows (-1, -1) and distance INT64_MAX.
 * Arithmetic: bytes are shifted to int8 (x ^ 0x80 = x - 128) and a frame pair's distance is |a'|^2 + |b'|^2 - 2 a'.b' (independent of the shift), the dot on
 * v_mfma_i32_32x32x32_i8 with an int32 accumulator — exact while K <= 65536 (128 * 128 * 65536 = 2^30) — and both norms int32 sums over the same loaded bytes;
 * bytes padded beyond K are zero AFTER the shift.  Clip distances are int64 sums of T uint32 frame distances.  No atomics; the chunking changes no output bit. */
/* Bytes of workspace dcv_clipnn_search needs for n queries when a call covers chunk_frames window starts: the running best (n k int64), the workgroups' candidates
 * (2 n k ceil(chunk_frames / 1024) int64) and the uint32 frame distances (n T rows of chunk_frames + T - 1 columns, rounded up to 64).  0 with dcv_last_error set
 * unless 1 <= n <= 65535, 1 <= T <= 4096, n T < 2^24, 1 <= k <= 8, 1 <= chunk_frames < 2^30.  Host arithmetic only. */
size_t dcv_clipnn_workspace_bytes(int n, int T, int k, int64_t chunk_frames);
/* Queries (n, C, T, H, W) with the element strides of xd, uint8 (is_f32 = 0: copied) or fp32 (is_f32 = 1: uint8((clip(x,-1,1)+1)/2*255) in dcv_videos_to_uint8's
 * fp32 operation order, bytes identical) -> out: n T frames of H*W*C bytes in disk order (H, W, C), contiguous.  One launch, one thread per byte.
 * DCV_EINVAL before the launch: a NULL pointer, is_f32 outside {0, 1}, an extent < 1, C > 4, fp32 data off a 4-byte boundary; DCV_EUNSUPPORTED: H*W*C > 65536. */
int dcv_clipnn_pack_queries(const void* x, int is_f32, const dcv_dims5* xd, uint8_t* out, void* stream);
/* One chunk of a search: window starts chunk_start .. chunk_start + chunk_frames - 1 of the packed buffer of F = starts[N] frames (a window start is a frame
 * index f with f + T <= F; those whose T frames span two videos are masked out).  A search is the calls chunk_start = 0, chunk_frames, 2 chunk_frames, ... while
 * chunk_start <= F - T, in that order, with the same arguments and workspace: the call with chunk_start = 0 starts the running best, the others merge into it, and
 * after the last one rows (n, k, 2) int32 = (video, t0) and dist (n, k) int64 hold the result — the same bits for every chunk_frames.
 * The query clips are `queries` (n T packed frames, dcv_clipnn_pack_queries) or, with queries NULL, the windows that the (n, 2) int32 table `qtable` names in the
 * store itself; a table row that names no T frames of one video is read as nothing and gets no window at all.  exclude: NULL, or query q excludes video
 * exclude[q * exclude_stride] (negative: none); qtable with stride 2 excludes each query's own video.
 * Three launches: the int8 GEMM (workgroups of 256 query frames x 64 store frames, grid over the chunk's frames and the query tiles; 16-byte fragment loads when
 * H*W*C % 16 == 0 and both buffers are on 16-byte boundaries, else unaligned and, in the last K step, single-byte loads), the diagonal sums with the per-workgroup
 * k best, the merge.  DCV_EINVAL before any launch: a NULL or misaligned pointer, both or neither of queries / qtable, an extent or count outside the limits of
 * dcv_clipnn_workspace_bytes, C outside 1..4, N or F outside [1, 2^31), F < T, chunk_start not a multiple of chunk_frames inside [0, F - T]; DCV_EUNSUPPORTED:
 * H*W*C > 65536; DCV_EWORKSPACE: fewer than dcv_clipnn_workspace_bytes bytes. */
int dcv_clipnn_search(const uint8_t* frames, const int64_t* starts, int64_t N, int64_t F, int T, int H, int W, int C, const uint8_t* queries, const int32_t* qtable, int n,
                      const int32_t* exclude, int exclude_stride, int k, int64_t chunk_start, int64_t chunk_frames, int32_t* rows, int64_t* dist, void* ws,
                      size_t ws_bytes, void* stream);
/* out (B, C, T, H, W) uint8 contiguous = the stored bytes of the table's windows of a uint8 stream (F, H, W, C): a copy, no arithmetic.  A row that names no T frames
 * of one video is written as zeros and nothing is read for it.  One launch.  DCV_EINVAL before it unless 1 <= B <= 65535, T, H, W >= 1, 1 <= C <= 4, 1 <= N < 2^31. */
int dcv_clipnn_gather_u8(const uint8_t* frames, const int32_t* table, const int64_t* starts, int64_t N, int B, int T, int H, int W, int C, uint8_t* out, void* stream);

/* ---- on-device evaluation statistics: Inception score, Frechet and kernel distance (added symbols only: the ABI version stays 4) ------ *
 * The reference's Trainer.evaluate (trainer.py:171-224) moves the generators to the CPU, writes every generated clip as an mp4 and lets an external package read
 * them back for IS / FID / PRD.  These entries are the dense arithmetic AFTER the feature network (which stays the caller's): they accumulate, in fp64 and in device
 * memory, what the three metrics are finalised from.  No floating-point atomic: every output element has one owning workgroup and every sum one order, so the same
 * sequence of calls gives the same bits.  Every refusal (DCV_EINVAL, DCV_EWORKSPACE) is returned before the first launch.
 *
 * Feature moments, the statistics of the Frechet distance (Heusel et al. 2017: mu = sum / n, Sigma = (gram - sum sum^T / n) / (n - 1)):
 *   sum[c] += sum_i x[i][c];   gram[c][d] += sum_i x[i][c] * x[i][d]        x: n rows of D fp32 values, row_stride >= D elements apart
 * Operands are converted to fp64 on load (a product of two fp32 values is exact in fp64) and go through v_mfma_f64_16x16x4_f64 with the stored values of the gram
 * tile as the accumulator input, rows in ascending order, four per instruction: the only rounding is the fp64 accumulation.  A 64 x 64 tile of gram has one owning
 * workgroup (the upper tiles are computed, the lower ones stored as their mirror image; inside a diagonal tile both halves are computed from the same products in
 * the same order): after every call gram is the full matrix, symmetric bit for bit.  sum: one lane per column, rows ascending.  A non-finite feature propagates.
 * The caller zeroes sum (D doubles) and gram (D x D doubles) once and keeps the row count.  One launch.  1 <= D <= 4096, 1 <= n < 2^31. */
int dcv_eval_moments_update(const float* x, int64_t n, int D, int64_t row_stride, double* sum, double* gram, void* stream);
/* The Inception score's sums (Salimans et al. 2016: IS = exp(E_x KL(p(y|x) || p(y))) = exp(sum_i sum_k p_ik log p_ik / n - sum_k pbar_k log pbar_k), pbar = sum_i p_i / n):
 *   state[k] += sum_i p_ik (k < K);   state[K] += sum_i sum_k p_ik log p_ik        logits: n rows of K fp32 values, row_stride >= K elements apart
 * Per row, in fp64, every operation rounded on its own: m = max_k z_k; e_k = exp(z_k - m); S = sum_k e_k; p_k = e_k / S; log p_k = (z_k - m) - log S; a class with
 * p_k == 0 adds nothing to the last sum.  Workgroup g of G = min(n, 256) takes rows g, g + G, ...; its 256 lanes hold classes l, l + 256, ... (S: lane order, then the
 * tree of dcv_lecam_sums) and leave K + 1 partial sums in row g of the workspace; a second launch adds the G rows in ascending g and then the state.  Two launches.
 * state: K + 1 doubles, zeroed once by the caller.  1 <= K <= 4096, 1 <= n < 2^31; workspace of at least dcv_eval_inception_workspace_bytes(n, K) (0: out of range). */
size_t dcv_eval_inception_workspace_bytes(int64_t n, int K);
int dcv_eval_inception_update(const float* logits, int64_t n, int K, int64_t row_stride, double* state, void* workspace, size_t workspace_bytes, void* stream);
/* The kernel distance (Binkowski et al. 2018; the subset protocol and the defaults of Karras et al. 2020, "Training generative adversarial networks with limited
 * data": 100 subsets of 1000, k(x, y) = (x.y / D + 1)^3).
 * dcv_eval_kid_draw writes the int32 table (subsets, 2, m): row (s, 0) = the first m images of a keyed permutation of [0, na), row (s, 1) of [0, nb):
 *   table[s][side][i] = perm(i), the bijection of dcv_clipstore_draw on [0, na or nb) with key {lo, hi} of seed + DCV_EVAL_KID_SALT and the Philox counter
 *   {R, r, s, side} in round r.  One launch, no state.  m <= na, nb < 2^31. */
#define DCV_EVAL_KID_SALT 0x9FB21C651E98DF25ull
int dcv_eval_kid_draw(int32_t* table, int subsets, int m, int64_t na, int64_t nb, uint64_t seed, void* stream);
/* For subset s, with a_i = fa[table[s][0][i]] and b_j = fb[table[s][1][j]] (rows of D fp32 values, stride_a / stride_b >= D elements apart):
 *   out[3 s + 0] = sum_{i != j} k(a_i, a_j);   out[3 s + 1] = sum_{i != j} k(b_i, b_j);   out[3 s + 2] = sum_{i, j} k(a_i, b_j)        in fp64
 * MMD^2_s = out0 / (m (m - 1)) + out1 / (m (m - 1)) - 2 out2 / m^2 is the host's.  The dot products run through v_mfma_f64_16x16x4_f64 with the contraction over D
 * (operands converted on load: exact products); the m x m kernel matrix is never written: per 64 x 64 tile the epilogue forms t = dot / D + 1, (t * t) * t — each
 * operation rounded on its own —, leaves out the diagonal of the two symmetric blocks, and reduces the tile to one partial in the workspace (only the upper tiles of
 * a symmetric block are computed; an off-diagonal one counts twice, exactly); a second launch sums a subset's partials in a fixed order.  Two launches.
 * A table entry outside [0, na) / [0, nb) is not followed: its row counts as NaN.  2 <= m <= 65536, 1 <= subsets <= 4096, 1 <= D <= 4096; workspace of at least
 * dcv_eval_kid_workspace_bytes(subsets, m) (0: out of range). */
size_t dcv_eval_kid_workspace_bytes(int subsets, int m);
int dcv_eval_kid_sums(const float* fa, int64_t stride_a, int64_t na, const float* fb, int64_t stride_b, int64_t nb, int D, const int32_t* table, int subsets, int m,
                      void* workspace, size_t workspace_bytes, double* out, void* stream);

/* ---- on-device evaluation: improved precision / recall and density / coverage (added symbols only: the ABI version stays 4) ---------- *
 * The k-nearest-neighbour manifold metrics (Kynkaanniemi et al. 2019; Naeem et al. 2020) over A = na real and B = nb fake rows of D fp32 features, row strides >= D:
 *   d2(x, y) = max(0, (|x|^2 + |y|^2) - 2 x.y)                      fp64, every operation rounded on its own; a NaN stays a NaN and compares false everywhere
 *   rad2_k(X)[i] = the k-th smallest d2(x_i, x_j) over j != i         self excluded by index: a duplicate row is a neighbour at distance 0
 *   precision = #{j : exists i, d2(b_j, a_i) <= rA[i]} / nb           recall = #{i : exists j, d2(a_i, b_j) <= rB[j]} / na
 *   density = sum_j #{i : d2(b_j, a_i) <= rA[i]} / (k nb)             coverage = #{i : min_j d2(a_i, b_j) <= rA[i]} / na
 * Every comparison is <=.  The dot products run through v_mfma_f64_16x16x4_f64 with the contraction over D, as in dcv_eval_kid_sums (64 x 64 tile per workgroup,
 * one 16-byte read per lane feeding four MFMAs where D, the strides and the bases allow it, four guarded 4-byte reads otherwise); the n x n distance matrix is never
 * written.  A workgroup owns 64 rows and a share of the column tiles (s, s + S, ...); what the shares leave is combined by operations that do not depend on the
 * order (the k smallest of a multiset, integer sums, minima), so every result is the same bits for every S.  No atomic.  col_splits = 0: the library chooses
 * S = max(1, min(64, column tiles, 512 / row tiles)) (tiles of 64); 1 .. 64 forces S.  1 <= D <= 4096, 1 <= k <= 16, fewer than 2^31 rows; every refusal
 * (DCV_EINVAL, DCV_EWORKSPACE) is returned before the first launch.
 *
 * norms[i] = sum_d x[i][d]^2 in fp64, features ascending.  One launch.  1 <= n < 2^31. */
int dcv_eval_row_norms(const float* x, int64_t n, int D, int64_t row_stride, double* norms, void* stream);
/* rad2[i] = rad2_k(X)[i] for the n rows of x with their norms (+inf where fewer than k distances are not NaN).  The first launch keeps, per row and share, the k
 * smallest d2 in the workspace (per tile the distances pass through one LDS tile and four lanes per row scan them into ascending lists in registers); the second
 * merges a row's S lists.  Two launches.  k + 1 <= n < 2^31; workspace of at least dcv_eval_knn_workspace_bytes(n, k, col_splits) = S * n * k * 8 (0: out of range). */
size_t dcv_eval_knn_workspace_bytes(int64_t n_rows, int k, int col_splits);
int dcv_eval_knn_radii(const float* x, int64_t n, int D, int64_t row_stride, const double* norms, int k, int col_splits, void* workspace, size_t workspace_bytes,
                       double* rad2, void* stream);
/* Per query row q of `queries` against the ns rows of `support` with the supports' rad2:
 *   count[q] = #{i : d2(q, s_i) <= rad2[i]}  (int32);   dmin2[q] = min_i d2(q, s_i)  (fp64; +inf if every distance is NaN)
 * rad2 may be null: count is then 0 and only dmin2 is formed (coverage alone).  The first launch leaves a count and a minimum per query and share in the workspace,
 * the second adds the counts and folds the minima.  Two launches.  1 <= nq, ns < 2^31, nq * ns < 2^53; workspace of at least
 * dcv_eval_manifold_workspace_bytes(nq, ns, col_splits) = S * nq * 12 (0: out of range). */
size_t dcv_eval_manifold_workspace_bytes(int64_t n_queries, int64_t n_support, int col_splits);
int dcv_eval_manifold_counts(const float* queries, int64_t stride_q, int64_t nq, const double* norms_q, const float* support, int64_t stride_s, int64_t ns,
                             const double* norms_s, const double* rad2, int D, int col_splits, void* workspace, size_t workspace_bytes, int32_t* count, double* dmin2,
                             void* stream);
/* The integers a metric is a ratio of, over the n query rows of one dcv_eval_manifold_counts call, as doubles (64-bit integer sums, exact below 2^53):
 *   out[0] = #{count > 0};  out[1] = sum count;  out[2] = #{dmin2 <= own_rad2} (0 when own_rad2 is null);  out[3] = #{norms not finite}
 * own_rad2: the QUERIES' own radii (coverage compares a real row's nearest fake with the real row's radius); norms: the queries' norms.  One launch, one workgroup. */
int dcv_eval_manifold_reduce(const int32_t* count, const double* dmin2, const double* own_rad2, const double* norms, int64_t n, double* out, void* stream);

/* ---- on-device evaluation: PRD, the k-means of the precision-recall curve (added symbols only: the ABI version stays 4) ---------------- *
 * The reference's third metric (trainer.py:216-219: "prd"; Sajjadi et al. 2018) clusters the UNION of the real rows A (na) and the fake rows B (nb) — D fp32 features,
 * row strides >= D; union row u is a_u for u < na, else b_{u - na}; n = na + nb < 2^31; the union is never copied together — and compares the two sides' cluster
 * histograms.  R independent runs of C clusters, full-batch Lloyd; the centroids are one (R, C, D) fp64 tensor.  1 <= C <= 64, C <= n, 1 <= R <= 64, 1 <= D <= 4096.
 * No floating-point atomic: one owner per output element and one order per sum.  Every refusal (DCV_EINVAL, DCV_EWORKSPACE) is returned before the first launch.
 *
 * Seeding (trainer.py:216-219): cent[r][c] = union row perm_r(c) as doubles, perm_r = the bijection of dcv_clipstore_draw on [0, n) with key {lo, hi} of
 * seed + DCV_EVAL_PRD_SALT and the Philox counter {R, round, r, 0}: the run where dcv_eval_kid_draw puts the subset.  A run's rows are distinct.  One launch. */
#define DCV_EVAL_PRD_SALT 0xC2B2AE3D27D4EB4Full
int dcv_eval_prd_seed(const float* fa, int64_t stride_a, int64_t na, const float* fb, int64_t stride_b, int64_t nb, int D, int C, int R, uint64_t seed, double* cent,
                      void* stream);
/* Assignment (trainer.py:216-219): cn[r][c] = sum_d cent[r][c][d]^2 (features ascending), score(u, r, c) = cn[r][c] - 2 x_u.cent[r][c] in fp64, every operation
 * rounded on its own; the dot runs through v_mfma_f64_16x16x4_f64 with the contraction over D in dcv_eval_knn_radii's order (fp32 features converted on load, fp64
 * centroids as they are; one 16-byte read of the features feeding four MFMAs where D, the strides and the bases allow it, guarded single reads otherwise).
 *   assign[r][u] (int32, (R, n)) = the LOWEST c of minimal score among the scores that are not NaN; C ("unassigned") where the row's norm (dcv_eval_row_norms of its
 *   side) is not finite or no score is comparable.
 * A workgroup owns 64 union rows and sweeps the runs — 4, 2 or 1 of them per 64-column tile for C <= 16, 32, 64 —: the rows are fetched once for all R runs.  Two launches (cn, the sweep); workspace of
 * at least dcv_eval_prd_assign_workspace_bytes(C, R) = R * C * 8 (0: out of range). */
size_t dcv_eval_prd_assign_workspace_bytes(int C, int R);
int dcv_eval_prd_assign(const float* fa, int64_t stride_a, int64_t na, const float* fb, int64_t stride_b, int64_t nb, const double* norms_a, const double* norms_b, int D,
                        const double* cent, int C, int R, int32_t* assign, void* workspace, size_t workspace_bytes, void* stream);
/* Counts (trainer.py:216-219): hist[r][side][c] (int32, (R, 2, C + 1); side 0 = real) = the side's rows with assign[r][u] == c; column C counts every other row, and
 * every row whose norm is not finite whatever its entry.  One launch. */
int dcv_eval_prd_count(const int32_t* assign, const double* norms_a, int64_t na, const double* norms_b, int64_t nb, int C, int R, int32_t* hist, void* stream);
/* Update (trainer.py:216-219): hist as dcv_eval_prd_count writes it; sum[r][c][d] = the fp64 sum of x_u[d] over the rows counted in hist[r][.][c]; then
 * cent[r][c][d] = sum / count (one division) where count > 0 — an empty cluster keeps its centroid bit for bit.  The sums are a GEMM with the contraction over the
 * union's rows on v_mfma_f64_16x16x4_f64, the A operand the selector assign[r][u] == c (a product of 0 / 1 and an fp32 value is exact); the rows are cut into S slabs
 * of ceil(n / S) rows rounded up to 16, a slab's rows added ascending (four per instruction) into the workspace and the slabs ascending by the last launch.
 * row_splits = 0: S = max(1, min(64, ceil(n / 64), 1024 / (ceil(R C / 64) * ceil(D / 64)))), from the shapes alone; 1 .. 64 forces S.  With integer features every
 * sum is exact and the result is the same bits for every S.  Three launches (counts, slab sums, fold); workspace of at least
 * dcv_eval_prd_update_workspace_bytes(n, D, C, R, row_splits) = S * R * C * D * 8 (0: out of range). */
size_t dcv_eval_prd_update_workspace_bytes(int64_t n, int D, int C, int R, int row_splits);
int dcv_eval_prd_update(const float* fa, int64_t stride_a, int64_t na, const float* fb, int64_t stride_b, int64_t nb, const double* norms_a, const double* norms_b,
                        const int32_t* assign, int D, int C, int R, int row_splits, double* cent, int32_t* hist, void* workspace, size_t workspace_bytes, void* stream);

/* ---- RunState: snapshot, fingerprint and restore of a run's state tensors (added symbols only: the ABI version stays 4) ---- *
 * Every tensor is handled as 32-bit words ("dwords": an fp32 or int32 element is one, an int64 element two), 0 <= dwords < 2^32 per tensor, on a 4-byte
 * boundary; a tensor without dwords is skipped (its digest is (0, 0)) and may be null.  Up to 24 tensors per launch (the multi-tensor table of DESIGN §10a), any
 * number per call; every check comes before the first launch.
 * The digest of w[0 .. n): with z = i * 0x9E3779B97F4A7C15 + w[i] (mod 2^64) and h_i = the splitmix64 finaliser of z (z ^= z >> 30; z *= 0xBF58476D1CE4E5B9;
 * z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31), the pair (sum of h_i mod 2^64, xor of h_i): exact and independent of the traversal.  `digests` is
 * n_tensors x 2 uint64 in device memory.  Per-block partial pairs go through `workspace`, at least dcv_state_workspace_bytes(n_tensors, dwords) bytes on an 8-byte
 * boundary (0: a size out of range), and one block per tensor folds them: two launches per table of 24 (one for a table without dwords).
 * dcv_state_pack_multi: tensor t's dwords -> arena[offsets[t] ..), the dwords up to the next multiple of 4 written as zero, and the digests in the same pass.  The
 * arena is on a 16-byte boundary; offsets are multiples of 4 dwords, ascending, the (padded) segments disjoint and inside arena_dwords.  16-byte accesses where
 * the source is on a 16-byte boundary too.
 * dcv_state_unpack_multi: the inverse copy (no digest, no workspace; one launch per table that has dwords).
 * dcv_state_digest_multi: the digests alone, of live tensors or of arena segments; nothing is written but digests and workspace. */
size_t dcv_state_workspace_bytes(int n_tensors, const int64_t* dwords);
int dcv_state_pack_multi(int n_tensors, const void* const* src, const int64_t* dwords, void* arena, int64_t arena_dwords, const int64_t* offsets,
                         uint64_t* digests, void* workspace, size_t workspace_bytes, void* stream);
int dcv_state_unpack_multi(int n_tensors, void* const* dst, const int64_t* dwords, const void* arena, int64_t arena_dwords, const int64_t* offsets, void* stream);
int dcv_state_digest_multi(int n_tensors, const void* const* src, const int64_t* dwords, uint64_t* digests, void* workspace, size_t workspace_bytes, void* stream);

/* ---- RunMonitor: the training log kept on the device (added symbols only: the ABI version stays 4) ---------------------------- *
 * The reference reads four losses on the host every iteration (trainer.py:326-328,363: logger.update("loss_*", loss.cpu().item())), averages them between
 * logger.log() calls (logger.py:144-148,280-283) and histograms / tiles its samples in numpy (trainer.py:109-169).  These entries keep all of that on the device.
 * The state is ONE tensor of 8-byte words in device memory, owned by the caller: a header, then n_slots scalar slots, then n_groups logit groups.  Fields marked
 * f64 hold the bits of a double, the others an int64.  A fresh state is all zero except every slot's MIN = +inf and MAX = -inf (and FIRST_ITERATION, the caller's). */
#define DCV_MONITOR_MAX_SLOTS 32
#define DCV_MONITOR_MAX_GROUPS 16
#define DCV_MONITOR_HEADER_WORDS 4
#define DCV_MONITOR_FIRST_ITERATION 0   /* i64: the first iteration of the window (the roll before it stamped iteration + 1)                    */
#define DCV_MONITOR_LAST_ITERATION 1    /* i64: in a record the iteration of its roll; in the live window that of the roll before               */
#define DCV_MONITOR_OBSERVATIONS 2      /* i64: dcv_monitor_observe calls in the window                                                         */
#define DCV_MONITOR_ROLLS 3             /* i64: rolls before this window: survives the reset and increments                                     */
#define DCV_MONITOR_SLOT_WORDS 6
#define DCV_MONITOR_SLOT_SUM 0          /* f64: sum of the finite values, in call order, one rounding per value                                 */
#define DCV_MONITOR_SLOT_COUNT 1        /* i64: finite values                                                                                   */
#define DCV_MONITOR_SLOT_NONFINITE 2    /* i64: inf / NaN values (left out of SUM, MIN, MAX)                                                    */
#define DCV_MONITOR_SLOT_MIN 3          /* f64: +inf while COUNT == 0                                                                           */
#define DCV_MONITOR_SLOT_MAX 4          /* f64: -inf while COUNT == 0                                                                           */
#define DCV_MONITOR_SLOT_LAST 5         /* f64: the last observed value, non-finite ones included                                               */
#define DCV_MONITOR_GROUP_WORDS 6
#define DCV_MONITOR_GROUP_N 0           /* i64: logits seen, non-finite ones included                                                           */
#define DCV_MONITOR_GROUP_SUM 1         /* f64: sum of the finite logits                                                                        */
#define DCV_MONITOR_GROUP_SUMSQ 2       /* f64: sum of (double)y * (double)y over the finite logits                                             */
#define DCV_MONITOR_GROUP_POS 3         /* i64: finite logits > 0 (+-0 counts in neither)                                                       */
#define DCV_MONITOR_GROUP_NEG 4         /* i64: finite logits < 0                                                                               */
#define DCV_MONITOR_GROUP_NONFINITE 5   /* i64: inf / NaN logits (left out of both sums and both sign counts)                                   */
/* trainer.py:326-328,363 + logger.py:144-148 (Logger.update).  slots[s]: a HOST table of n_slots pointers to fp32 device scalars; NULL = not observed this
 * iteration.  A finite v: SUM = SUM + (double)v (one rounding), COUNT += 1, MIN / MAX by `<` / `>` on doubles; a non-finite v: NONFINITE += 1; LAST = (double)v
 * either way.  groups[g]: a HOST table of n_groups contiguous fp32 device tensors of group_n[g] elements, 1 <= n <= 2^24; NULL = skipped.  Per group the batch
 * sums S = sum (double)y and Q = sum (double)y * (double)y over the finite elements in dcv_lecam_sums' order (256 lanes, lane l adds elements l, l + 256, ... into
 * a double that starts at +0.0; then p[l] += p[l + s] for s = 128 .. 1), then SUM = SUM + S and SUMSQ = SUMSQ + Q, one rounding each; POS, NEG, NONFINITE and N
 * are exact integer counts.  OBSERVATIONS += 1.  One launch: one workgroup per group plus one for the scalars; no atomics; nothing but the state is written.
 * DCV_EINVAL before any launch unless 0 <= n_slots <= 32, 0 <= n_groups <= 16, no needed table NULL, the state non-null on an 8-byte boundary. */
int dcv_monitor_observe(int n_slots, const float* const* slots, int n_groups, const float* const* groups, const int64_t* group_n, int64_t* state, void* stream);
/* logger.py:280-283 (Logger.log: publish the averages' ingredients, start over).  record[i] = state[i] for every word, with record[LAST_ITERATION] = iteration;
 * then the window is reset: every slot's MIN = +inf, MAX = -inf, every other slot and group word 0, OBSERVATIONS = 0, FIRST_ITERATION = iteration + 1,
 * LAST_ITERATION = iteration, ROLLS += 1.  `record`: 4 + 6 n_slots + 6 n_groups words of device memory on an 8-byte boundary, not the state.  One launch. */
int dcv_monitor_roll(int n_slots, int n_groups, int64_t* state, int64_t* record, int64_t iteration, void* stream);
/* trainer.py:134-135,159-160 (tf_log_histgram(x[:, 0])): counts[b] (+)= the number of bytes equal to b in channel `channel` of the contiguous uint8 tensor
 * x (N, C, T, H, W); counts: 256 int64 in device memory.  accumulate = 0 overwrites counts (one more launch that zeroes them), otherwise adds (batched sampling).
 * A workgroup takes up to 16 KiB of one clip's run of T*H*W bytes: 16-byte loads between the run's 16-byte boundaries, single bytes before and after (runs start
 * misaligned whenever C*T*H*W % 16 != 0); counters privatised per wave in LDS, equal neighbouring bytes folded into one add; one 64-bit global atomic add per
 * non-empty bin and workgroup.  Integer adds commute: exact.  DCV_EINVAL before any launch for an extent < 1, channel outside [0, C), a NULL pointer. */
int dcv_hist_u8(const uint8_t* x, int N, int C, int T, int H, int W, int channel, int64_t* counts, int accumulate, void* stream);
/* trainer.py:138-143,163-168 (make_video_grid twice, np.concatenate on the last axis, transpose(0, 2, 1, 3, 4)) as one gather: geo, colour: contiguous uint8
 * (N, 3, T, H, W), N = rows * cols; out: contiguous uint8 (1, T, 3, rows*H, 2*cols*W); clip r*cols + c lands in cell (r, c) of its half, geo on the left.
 * 16-byte copies when W % 16 == 0 and all three pointers are on 16-byte boundaries, single bytes otherwise.  One launch. */
int dcv_video_grid_u8(const uint8_t* geo, const uint8_t* colour, int rows, int cols, int N, int T, int H, int W, uint8_t* out, void* stream);

/* ---- bf16 channels-last ("CL16") data path -------------------------------------------------- *
 * BASELINE.json configs[2] ("surreal-depth1, bf16 MFMA") and configs[4] ("fp16 MFMA") name 16-bit variants of the same step
 * (config/surreal-depth1.yml:5,47-76, config/isogd-flow.yml; the reference itself is fp32-only).  This is that path as a DATA path:
 * activations and their gradients are bf16 in HBM with the channel innermost (memory order n, d, h, w, c: `sc` = 1, the pixel pitch
 * a multiple of 8 elements and >= the channel count rounded up to 8 — padding channels hold zeros), so an MFMA operand fragment
 * (8 consecutive k = channels of one tap) is one 16-byte read for every stride / padding; weights stay fp32 masters in torch layout
 * (packed to bf16 K-major tiles by dcv_cl_pack_weights, once per optimiser step), accumulators, BatchNorm statistics, weight gradients and
 * the optimiser stay fp32.  v_mfma_f32_32x32x16_bf16.  Same call sites as the fp32 entry points above; `void*` tensors are bf16,
 * described by dcv_dims5 with element strides.  A throughput path with its own tolerance (tests/test_cl16_gpu.py), never the default. */
size_t dcv_cl_packed_bytes(const dcv_conv_geom* g, const dcv_dims5* x, const dcv_dims5* y, int which /*0 fwd, 1 bwd-data*/);
int dcv_cl_pack_weights(const dcv_conv_geom* g, const dcv_dims5* x, const dcv_dims5* y, int which, const float* w, void* packed, size_t bytes, void* stream);
/* scratch a forward / backward-data call REQUIRES (thin destinations — <= 8 channels fed by a wide source — run as a 1x1 GEMM over the source followed by a gather
 * of each destination pixel's taps, and keep the GEMM's result there; the latent layers' split-K form keeps its fp32 partial sums there): a call given less is
 * refused with DCV_EWORKSPACE before any launch.  Likewise dcv_cl_pack_weights with fewer than dcv_cl_packed_bytes. */
size_t dcv_cl_conv_workspace_bytes(const dcv_conv_geom* g, const dcv_dims5* x, const dcv_dims5* y, int which);
int dcv_cl_conv_forward(const dcv_conv_geom* g, const void* x, const dcv_dims5* xd, const void* packed, void* y, const dcv_dims5* yd,
                        int act, float slope, void* ws, size_t ws_bytes, void* stream);
/* conv -> BatchNorm pairs in training mode (as dcv_conv_forward_stats on the fp32 path): the epilogue also leaves {sum, sum of squares} of the STORED bf16 values per position tile
 * and output channel: *nparts rows of *pitch channels x 2 floats in `stat` (dcv_cl_conv_stats_bytes; 0 = this geometry's form produces none, and *nparts stays 0: the BatchNorm op
 * then makes its own pass).  dcv_cl_bn_act_forward_stats consumes them. */
size_t dcv_cl_conv_stats_bytes(const dcv_conv_geom* g, const dcv_dims5* x, const dcv_dims5* y);
int dcv_cl_conv_forward_stats(const dcv_conv_geom* g, const void* x, const dcv_dims5* xd, const void* packed, void* y, const dcv_dims5* yd,
                              float* stat, size_t stat_bytes, int* nparts, int* pitch, void* ws, size_t ws_bytes, void* stream);
/* Rounding: every 16-bit value a convolution stores is ONE round-to-nearest-even of its fp32 accumulator (after the fused activation).  accumulate = 1 on the
 * tiled gather form (cl_gather_kernel with the row-order store, the form every thick layer takes) adds the old dx to that STORED rounding and rounds the sum again,
 * dx = rne16(rne16(conv^T(dy, w)) + dx_old) — bit for bit what storing the gradient and adding the two 16-bit tensors (dcv_cl_elementwise kind 1) gives, and up to one
 * 16-bit ulp from rne16(conv^T + dx_old) where both roundings land on ties; the gate of dcv_cl_conv_backward_data_gated multiplies that sum before the last rounding.
 * The thin-destination form (1x1 GEMM + cl_col2im_kernel) and the gather's direct 8-byte store form (a destination that is no whole 8-channel group) add dx_old in
 * fp32 and round once.  tests/test_conv_exact_gpu.py holds each form to its definition bit for bit. */
int dcv_cl_conv_backward_data(const dcv_conv_geom* g, const void* dy, const dcv_dims5* dyd, const void* packed, void* dx, const dcv_dims5* dxd,
                              int accumulate, void* ws, size_t ws_bytes, void* stream);
/* backward_data + the (Leaky)ReLU derivative of the layer that produced this convolution's input, read off that input `xg` (dx's shape and strides), in one epilogue
 * (ABI 3): dx = (accumulate ? dx : 0) + conv^T(dy, w); dx *= (xg > 0 ? 1 : slope).  The bf16 counterpart of dcv_conv_backward_data_gated (Inconv -> DownBlock 0,
 * generator.py:173-176,203-207).  DCV_EUNSUPPORTED before any launch where the form has no such epilogue. */
int dcv_cl_conv_backward_data_gated(const dcv_conv_geom* g, const void* dy, const dcv_dims5* dyd, const void* packed, void* dx, const dcv_dims5* dxd,
                                    int accumulate, const void* xg, const dcv_dims5* xgd, int act, float slope, void* ws, size_t ws_bytes, void* stream);
size_t dcv_cl_wgrad_workspace_bytes(const dcv_conv_geom* g, const dcv_dims5* x, const dcv_dims5* y);
int dcv_cl_conv_backward_weight(const dcv_conv_geom* g, const void* x, const dcv_dims5* xd, const void* dy, const dcv_dims5* dyd, float* dw,
                                void* ws, size_t ws_bytes, void* stream);
/* dw = (accumulate ? dw : 0) + corr(x, dy)  (ABI 3; as dcv_conv_backward_weight_acc) */
int dcv_cl_conv_backward_weight_acc(const dcv_conv_geom* g, const void* x, const dcv_dims5* xd, const void* dy, const dcv_dims5* dyd, float* dw, int accumulate,
                                    void* ws, size_t ws_bytes, void* stream);
/* module boundary: fp32 NCDHW (any strides) <-> bf16 channels-last (same shape; padding channels are written as zeros).
 * dcv_cl_to_f32 with accumulate = 1 adds into y (a gradient arriving at an fp32 leaf). */
int dcv_cl_from_f32(const float* x, const dcv_dims5* xd, void* y, const dcv_dims5* yd, void* stream);
int dcv_cl_to_f32(const void* x, const dcv_dims5* xd, float* y, const dcv_dims5* yd, int accumulate, void* stream);
/* kind 0: y = x   1: y = a x + b z   2: y = x + a N(0,1) (Philox; discriminator.py:30-39)   3: dx = x * lrelu'(z; slope a) (x = dy, z = the activation's output)
 * 4: dx = x * (1 - z^2) (tanh, z = output)   5: y = lrelu(x; a)   6: y = tanh(x) */
int dcv_cl_elementwise(int kind, const void* x, const dcv_dims5* xd, const void* z, const dcv_dims5* zd, void* y, const dcv_dims5* yd,
                       float a, float b, uint64_t seed, uint64_t offset, void* stream);
/* BatchNorm{2,3}d (+ Dropout2d mask) (+ (Leaky)ReLU) on bf16 channels-last tensors; statistics, parameters and their gradients fp32
 * (generator.py:62-72,205-211,242-248; discriminator.py:96-100,191-202,290-302).  Same semantics as dcv_bn_act_forward / _backward. */
size_t dcv_cl_bn_workspace_bytes(int channels);
int dcv_cl_bn_act_forward(const void* x, const dcv_dims5* xd, void* y, const dcv_dims5* yd, const float* gamma, const float* beta,
                          float* running_mean, float* running_var, int64_t* num_batches_tracked, float* save_mean, float* save_invstd,
                          const float* mask, int training, float momentum, float eps, int act, float slope, void* ws, size_t ws_bytes, void* stream);
int dcv_cl_bn_act_forward_stats(const void* x, const dcv_dims5* xd, void* y, const dcv_dims5* yd, const float* gamma, const float* beta,
                                float* running_mean, float* running_var, int64_t* num_batches_tracked, float* save_mean, float* save_invstd,
                                const float* mask, float momentum, float eps, int act, float slope, const float* stat, int nparts, int pitch,
                                void* ws, size_t ws_bytes, void* stream);
int dcv_cl_bn_act_backward(const void* dy, const dcv_dims5* dyd, const void* x, const dcv_dims5* xd, void* dx, const dcv_dims5* dxd,
                           const float* gamma, const float* beta, const float* save_mean, const float* save_invstd, const float* mask,
                           int training, int act, float slope, float* dgamma, float* dbeta, void* ws, size_t ws_bytes, void* stream);


/* ---- the same 16-bit channels-last path with fp16 as its element type (ABI 3) ------------ *
 * BASELINE configs[4] names "fp16 MFMA" (config/isogd-flow.yml on 32 x 128 x 128 clips: the size-agnostic discriminators, discriminator.py:181-206,288-305).
 * conv_cl16.hip / cl_elementwise.hip are compiled a second time with _Float16 as the element type and v_mfma_f32_32x32x16_f16: identical layout, kernels and
 * semantics, 10 mantissa bits instead of 7, largest finite value 65504 (a pre-BatchNorm sum beyond it becomes inf: the stress leg of bench.py reports the
 * largest magnitude it saw).  Same signatures as the dcv_cl_* entry points above; tensors are torch.float16 on the host side. */
size_t dcv_clf16_packed_bytes(const dcv_conv_geom* g, const dcv_dims5* x, const dcv_dims5* y, int which );
size_t dcv_clf16_conv_workspace_bytes(const dcv_conv_geom* g, const dcv_dims5* x, const dcv_dims5* y, int which);
int dcv_clf16_pack_weights(const dcv_conv_geom* g, const dcv_dims5* x, const dcv_dims5* y, int which, const float* w, void* packed, size_t bytes, void* stream);
int dcv_clf16_conv_forward(const dcv_conv_geom* g, const void* x, const dcv_dims5* xd, const void* packed, void* y, const dcv_dims5* yd, int act, float slope, void* ws, size_t ws_bytes, void* stream);
size_t dcv_clf16_conv_stats_bytes(const dcv_conv_geom* g, const dcv_dims5* x, const dcv_dims5* y);
int dcv_clf16_conv_forward_stats(const dcv_conv_geom* g, const void* x, const dcv_dims5* xd, const void* packed, void* y, const dcv_dims5* yd, float* stat, size_t stat_bytes, int* nparts, int* pitch, void* ws, size_t ws_bytes, void* stream);
int dcv_clf16_conv_backward_data(const dcv_conv_geom* g, const void* dy, const dcv_dims5* dyd, const void* packed, void* dx, const dcv_dims5* dxd, int accumulate, void* ws, size_t ws_bytes, void* stream);
int dcv_clf16_conv_backward_data_gated(const dcv_conv_geom* g, const void* dy, const dcv_dims5* dyd, const void* packed, void* dx, const dcv_dims5* dxd, int accumulate, const void* xg, const dcv_dims5* xgd, int act, float slope, void* ws, size_t ws_bytes, void* stream);
size_t dcv_clf16_wgrad_workspace_bytes(const dcv_conv_geom* g, const dcv_dims5* x, const dcv_dims5* y);
int dcv_clf16_conv_backward_weight(const dcv_conv_geom* g, const void* x, const dcv_dims5* xd, const void* dy, const dcv_dims5* dyd, float* dw, void* ws, size_t ws_bytes, void* stream);
int dcv_clf16_conv_backward_weight_acc(const dcv_conv_geom* g, const void* x, const dcv_dims5* xd, const void* dy, const dcv_dims5* dyd, float* dw, int accumulate, void* ws, size_t ws_bytes, void* stream);
int dcv_clf16_from_f32(const float* x, const dcv_dims5* xd, void* y, const dcv_dims5* yd, void* stream);
int dcv_clf16_to_f32(const void* x, const dcv_dims5* xd, float* y, const dcv_dims5* yd, int accumulate, void* stream);
int dcv_clf16_elementwise(int kind, const void* x, const dcv_dims5* xd, const void* z, const dcv_dims5* zd, void* y, const dcv_dims5* yd, float a, float b, uint64_t seed, uint64_t offset, void* stream);
size_t dcv_clf16_bn_workspace_bytes(int channels);
int dcv_clf16_bn_act_forward(const void* x, const dcv_dims5* xd, void* y, const dcv_dims5* yd, const float* gamma, const float* beta, float* running_mean, float* running_var, int64_t* num_batches_tracked, float* save_mean, float* save_invstd, const float* mask, int training, float momentum, float eps, int act, float slope, void* ws, size_t ws_bytes, void* stream);
int dcv_clf16_bn_act_forward_stats(const void* x, const dcv_dims5* xd, void* y, const dcv_dims5* yd, const float* gamma, const float* beta, float* running_mean, float* running_var, int64_t* num_batches_tracked, float* save_mean, float* save_invstd, const float* mask, float momentum, float eps, int act, float slope, const float* stat, int nparts, int pitch, void* ws, size_t ws_bytes, void* stream);
int dcv_clf16_bn_act_backward(const void* dy, const dcv_dims5* dyd, const void* x, const dcv_dims5* xd, void* dx, const dcv_dims5* dxd, const float* gamma, const float* beta, const float* save_mean, const float* save_invstd, const float* mask, int training, int act, float slope, float* dgamma, float* dbeta, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DCVGAN_HIP_H */
