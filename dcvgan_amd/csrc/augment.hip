// Adaptive clip augmentation in front of the discriminators, fp32, gfx950: flip / integer translation / cutout / brightness-contrast of a whole clip
// as ONE exact gather (aug_rows_kernel), its adjoint (the same kernel, BWD), the per-clip parameter table drawn on the device (aug_draw_kernel) and the ADA
// probability kept in a device state block (aug_observe_kernel, aug_adjust_kernel).  No atomics, no interpolation, no host read: the same inputs give the same bits.
// The second half adds interpolated warps and saturation behind entries of their own (aug_warp_kernel, aug_warp_draw_kernel, the (B, 24) row): bilinear
// taps and a gather adjoint, still without atomics and with every sum in one order; the kernels above are what they were.
#include "dcv_common.h"
#include <algorithm>

namespace dcv {

typedef float aug_f4 __attribute__((ext_vector_type(4)));
typedef uint32_t aug_u4 __attribute__((ext_vector_type(4)));

// Every fp32 operation of this file is rounded on its own, never fused into a multiply-add: hipcc contracts a * b + c by default, and the specification (the
// numpy restatement in tests/test_augment_cpu.py reproduces every bit) is mul, round, add, round.
#pragma clang fp contract(off)
__device__ __forceinline__ float aug_mul(float a, float b) { return a * b; }
__device__ __forceinline__ float aug_mul_add(float a, float b, float c) {
    const float m = a * b;
    return m + c;
}

// One operand of the gather: any strided (B, C, T, H, W) view (the frame cotangent: T = 1)
struct AugSrc {
    const float* p;
    int64_t sn, sc, sd, sh, sw;
    int32_t on, vld;           // present; 16-byte loads are possible (base and pitches)
};

struct AugArgs {
    AugSrc src[2];             // FWD: src[0] is the clip.  BWD: up to two cotangents of the whole augmented clip
    AugSrc frame;              // BWD: the cotangent of frame `tf` of the augmented clip
    AugSrc base;               // BWD: a gradient that is already in the clip's own space; the sum starts from it
    float* y;                  // FWD: the augmented clip; BWD: the clip's gradient
    int64_t osn, osc, osd, osh, osw;
    const int32_t* table;      // (B, 8)
    int32_t C, T, H, W;
    int32_t colour, neg_ch, tf;
    int32_t ppw, wgs_per_clip; // planes a workgroup owns, workgroups per clip
    int32_t quad;              // a lane owns 4 consecutive output pixels (W % 4 == 0, every w stride 1); else one pixel
    int32_t vst;               // 16-byte stores are possible
    FastDiv div_gpr;           // groups per row
};

// The clip's row of the table, as the gather sees it.  Both directions read input column acol + s * ow of input row oh + rdy for output pixel (oh, ow):
//   FWD  y[h, w] = x[h - dy, flip ? W - 1 - (w - dx) : w - dx]            BWD  dx[hs, wsrc] = dy[hs + dy, (flip ? W - 1 - wsrc : wsrc) + dx]
// and the cutout box is tested at the AUGMENTED clip's pixel: the output's in FWD, the input's in BWD.
struct AugRow {
    int s, acol, rdy;
    int64_t cy0, cy1, cx0, cx1;
    float gain, bias;
    bool flip, aligned;        // aligned: dx % 4 == 0 and no flip -> a lane's four input columns are one aligned group, in range together
};

// the four (or one) input values of a lane from one operand, as bits; 0 where the pixel is out of range
template <int NV>
__device__ __forceinline__ void aug_gather(const AugSrc& s, bool aligned, int64_t off, const int (&iw)[NV], const bool (&inr)[NV], uint32_t (&v)[NV]) {
    const float* xin = s.p + off;
    if (NV == 4 && aligned && s.vld) {      // wave-uniform
        if (inr[0]) {
            const aug_u4 q = *reinterpret_cast<const aug_u4*>(xin + iw[0]);      // (as words: a bit cast of a vector ELEMENT lvalue reads element 0 whatever the index)
#pragma unroll
            for (int j = 0; j < NV; ++j) v[j] = q[j];
        } else {
#pragma unroll
            for (int j = 0; j < NV; ++j) v[j] = 0u;
        }
    } else {
#pragma unroll
        for (int j = 0; j < NV; ++j) v[j] = inr[j] ? __builtin_bit_cast(uint32_t, xin[(int64_t)iw[j] * s.sw]) : 0u;
    }
}

template <bool BWD, int NV>
__device__ __forceinline__ void aug_body(const AugArgs& a, const AugRow& r, int b, int p0, int p1) {
    const int H = a.H, W = a.W;
    const int gpr = (int)a.div_gpr.div, groups = H * gpr;
    const int c0 = p0 / a.T, t0 = p0 - c0 * a.T;
    for (int g = threadIdx.x; g < groups; g += 256) {
        const int oh = (int)fdiv((uint32_t)g, a.div_gpr), ow0 = (g - oh * gpr) * NV;
        const int ih = oh + r.rdy;
        const bool rowok = (unsigned)ih < (unsigned)H;
        const int ihc = rowok ? ih : 0;
        int iw[NV];
        bool inr[NV], ok[NV];
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int ow = ow0 + j;
            iw[j] = r.acol + r.s * ow;
            inr[j] = rowok && (unsigned)iw[j] < (unsigned)W;
            const int64_t ch = BWD ? ih : oh, cw = BWD ? iw[j] : ow;
            ok[j] = inr[j] && !(ch >= r.cy0 && ch < r.cy1 && cw >= r.cx0 && cw < r.cx1);
        }
        int c = c0, t = t0;
        for (int p = p0; p < p1; ++p) {
            const uint32_t sign = (r.flip && c == a.neg_ch) ? 0x80000000u : 0u;
            float o[NV];
            bool have = false;
            if (BWD && a.base.on) {
                const float* z = a.base.p + (int64_t)b * a.base.sn + (int64_t)c * a.base.sc + (int64_t)t * a.base.sd + (int64_t)oh * a.base.sh;
#pragma unroll
                for (int j = 0; j < NV; ++j) o[j] = z[(int64_t)(ow0 + j) * a.base.sw];
                have = true;
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const AugSrc& s = k < 2 ? a.src[k] : a.frame;
                if (!s.on || (!BWD && k > 0) || (k == 2 && t != a.tf)) continue;      // workgroup-uniform
                uint32_t v[NV];
                aug_gather<NV>(s, r.aligned, (int64_t)b * s.sn + (int64_t)c * s.sc + (k == 2 ? 0 : (int64_t)t * s.sd) + (int64_t)ihc * s.sh, iw, inr, v);
#pragma unroll
                for (int j = 0; j < NV; ++j) {
                    const float sv = __builtin_bit_cast(float, v[j] ^ sign);      // negation is exact, a NaN payload included
                    const float val = !a.colour ? sv : (BWD ? aug_mul(r.gain, sv) : aug_mul_add(sv, r.gain, r.bias));
                    const float term = ok[j] ? val : 0.f;
                    o[j] = have ? o[j] + term : term;      // the sum runs in the operands' order: base, src[0], src[1], frame
                }
                have = true;
            }
            if (!have) {
#pragma unroll
                for (int j = 0; j < NV; ++j) o[j] = 0.f;
            }
            float* yout = a.y + (int64_t)b * a.osn + (int64_t)c * a.osc + (int64_t)t * a.osd + (int64_t)oh * a.osh;
            if (NV == 4 && a.vst) {
                const aug_f4 q = {o[0], o[1], o[2], o[3]};
                *reinterpret_cast<aug_f4*>(yout + ow0) = q;
            } else {
#pragma unroll
                for (int j = 0; j < NV; ++j) yout[(int64_t)(ow0 + j) * a.osw] = o[j];
            }
            if (++t == a.T) { t = 0; ++c; }
        }
    }
}

template <bool BWD>
__global__ __launch_bounds__(256) void aug_rows_kernel(AugArgs a) {
    const int b = (int)(blockIdx.x / (uint32_t)a.wgs_per_clip);      // workgroup-uniform: the table row arrives by scalar loads
    const int run = (int)blockIdx.x - b * a.wgs_per_clip;
    const int32_t* __restrict__ row = a.table + (int64_t)b * 8;
    const int H = a.H, W = a.W;
    AugRow r;
    r.flip = row[0] != 0;
    // a shift of a whole plane or more leaves nothing in range: clamping keeps every index computation inside 32 bits for any table
    const int dx = min(max(row[1], -W), W), dy = min(max(row[2], -H), H);
    r.cy0 = row[3]; r.cx0 = row[4];
    r.cy1 = r.cy0 + (int64_t)row[5]; r.cx1 = r.cx0 + (int64_t)row[5];
    r.gain = a.colour ? __builtin_bit_cast(float, row[6]) : 1.f;
    r.bias = a.colour ? __builtin_bit_cast(float, row[7]) : 0.f;
    r.s = r.flip ? -1 : 1;
    r.acol = r.flip ? W - 1 + dx : (BWD ? dx : -dx);
    r.rdy = BWD ? dy : -dy;
    r.aligned = !r.flip && (dx % 4 == 0);
    const int p0 = run * a.ppw, p1 = min(p0 + a.ppw, a.C * a.T);
    if (a.quad) aug_body<BWD, 4>(a, r, b, p0, p1);
    else aug_body<BWD, 1>(a, r, b, p0, p1);
}

static const int AUG_MAX_HW = 4096;      // H and W up to this: pixel indices of a plane stay far inside 32 bits

static bool aug_w_unit(const dcv_dims5& d) { return d.w == 1 || d.sw == 1; }
static bool aug_vec_ok(const void* p, const dcv_dims5& d) {
    return reinterpret_cast<uintptr_t>(p) % 16 == 0 && d.sn % 4 == 0 && d.sc % 4 == 0 && d.sd % 4 == 0 && d.sh % 4 == 0;
}
static AugSrc aug_src(const float* p, const dcv_dims5* d) {
    AugSrc s;
    memset(&s, 0, sizeof(s));
    if (!p) return s;
    s.p = p; s.sn = d->sn; s.sc = d->sc; s.sd = d->sd; s.sh = d->sh; s.sw = d->sw;
    s.on = 1; s.vld = aug_vec_ok(p, *d) ? 1 : 0;
    return s;
}

// base, dy1, dyf may be NULL.  Every check comes before the launch (the v1 and the interpolating entries share them).
static int aug_check(const char* who, bool bwd, const float* base, const dcv_dims5* based, const float* x, const dcv_dims5* xd, const float* x1, const dcv_dims5* x1d,
                     const float* xf, const dcv_dims5* xfd, int frame, const int32_t* table, int table_rows, float* y, const dcv_dims5* yd) {
    if (!table || !y || !yd) return fail(DCV_EINVAL, "%s: null argument", who);
    if (!x && !x1 && !xf) return fail(DCV_EINVAL, "%s: no input", who);
    if ((x && !xd) || (x1 && !x1d) || (xf && !xfd) || (base && !based)) return fail(DCV_EINVAL, "%s: a tensor without its dimensions", who);
    if (yd->n < 1 || yd->c < 1 || yd->d < 1 || yd->h < 1 || yd->w < 1) return fail(DCV_EINVAL, "%s: empty tensor", who);
    if ((x && !same_shape(*xd, *yd)) || (x1 && !same_shape(*x1d, *yd)) || (base && !same_shape(*based, *yd)))
        return fail(DCV_EINVAL, "%s: input and output shapes differ", who);
    if (xf && (xfd->n != yd->n || xfd->c != yd->c || xfd->d != 1 || xfd->h != yd->h || xfd->w != yd->w || frame < 0 || frame >= yd->d))
        return fail(DCV_EINVAL, "%s: the frame cotangent must be (N, C, 1, H, W) of a frame inside the clip", who);
    if (table_rows != yd->n) return fail(DCV_EINVAL, "%s: the table has %d rows, the batch %d clips", who, table_rows, yd->n);
    if (yd->h > AUG_MAX_HW || yd->w > AUG_MAX_HW) return fail(DCV_EUNSUPPORTED, "%s: H and W up to %d (got %d x %d)", who, AUG_MAX_HW, yd->h, yd->w);
    const int64_t hw = (int64_t)yd->h * yd->w, planes = (int64_t)yd->c * yd->d;
    if (!bwd) {      // the augmented clip is a fresh contiguous NCDHW tensor (size-1 dimensions may carry any stride)
        const int64_t want[5] = {planes * hw, (int64_t)yd->d * hw, hw, yd->w, 1};
        const int64_t have[5] = {yd->sn, yd->sc, yd->sd, yd->sh, yd->sw};
        const int32_t size[5] = {yd->n, yd->c, yd->d, yd->h, yd->w};
        for (int i = 0; i < 5; ++i)
            if (size[i] > 1 && have[i] != want[i]) return fail(DCV_EINVAL, "%s: the output must be contiguous (N, C, D, H, W)", who);
    }
    if (planes >= (1 << 24)) return fail(DCV_EUNSUPPORTED, "%s: too many planes per clip", who);
    const void* ptrs[6] = {x, x1, xf, base, y, table};
    for (const void* p : ptrs)
        if (reinterpret_cast<uintptr_t>(p) % 4) return fail(DCV_EINVAL, "%s: pointers need 4-byte alignment", who);
    return DCV_OK;
}

static int aug_launch(const char* who, bool bwd, const float* base, const dcv_dims5* based, const float* x, const dcv_dims5* xd, const float* x1, const dcv_dims5* x1d,
                      const float* xf, const dcv_dims5* xfd, int frame, const int32_t* table, int table_rows, float* y, const dcv_dims5* yd, int colour, int neg_ch,
                      void* stream) {
    if (const int rc = aug_check(who, bwd, base, based, x, xd, x1, x1d, xf, xfd, frame, table, table_rows, y, yd)) return rc;
    if (neg_ch < -1 || neg_ch >= yd->c) return fail(DCV_EINVAL, "%s: flip_negate_channel %d of %d channels", who, neg_ch, yd->c);
    const int64_t planes = (int64_t)yd->c * yd->d;
    AugArgs a;
    memset(&a, 0, sizeof(a));
    a.src[0] = aug_src(x, xd); a.src[1] = aug_src(x1, x1d); a.frame = aug_src(xf, xfd); a.base = aug_src(base, based);
    a.tf = frame;
    a.y = y; a.table = table;
    a.osn = yd->sn; a.osc = yd->sc; a.osd = yd->sd; a.osh = yd->sh; a.osw = yd->sw;
    a.C = yd->c; a.T = yd->d; a.H = yd->h; a.W = yd->w;
    a.colour = colour ? 1 : 0; a.neg_ch = neg_ch;
    // ~2048 workgroups or more where the batch has them; a workgroup keeps one clip, hence one table row
    int64_t ppw = ((int64_t)yd->n * planes + 2047) / 2048;
    ppw = std::min<int64_t>(std::max<int64_t>(ppw, 1), planes);
    a.ppw = (int32_t)ppw;
    a.wgs_per_clip = (int32_t)((planes + ppw - 1) / ppw);
    const int64_t grid = (int64_t)yd->n * a.wgs_per_clip;
    if (grid >= (1ll << 31)) return fail(DCV_EUNSUPPORTED, "%s: too many workgroups", who);
    a.quad = (yd->w % 4 == 0 && aug_w_unit(*yd) && (!x || aug_w_unit(*xd)) && (!x1 || aug_w_unit(*x1d)) && (!xf || aug_w_unit(*xfd)) && (!base || aug_w_unit(*based))) ? 1 : 0;
    a.vst = (a.quad && aug_vec_ok(y, *yd)) ? 1 : 0;      // W % 4 == 0: every output row then starts on a 16-byte boundary
    a.div_gpr = make_fastdiv((uint32_t)(a.quad ? yd->w / 4 : yd->w));
    if (bwd) hipLaunchKernelGGL(aug_rows_kernel<true>, dim3((unsigned)grid), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    else hipLaunchKernelGGL(aug_rows_kernel<false>, dim3((unsigned)grid), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    DCV_LAUNCH_CHECK();
    return DCV_OK;
}

// ---- the table: one thread per clip ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float aug_u01(uint32_t r) { return ((float)r + 0.5f) * 2.3283064365386963e-10f; }      // the library's uniform, (0, 1]

__device__ __forceinline__ void aug_philox_block(uint64_t idx, uint64_t seed, uint64_t offset, uint32_t (&w)[4]) {
    uint32_t c[4] = {(uint32_t)idx, (uint32_t)(idx >> 32), (uint32_t)offset, (uint32_t)(offset >> 32)};
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
#pragma unroll
    for (int i = 0; i < 4; ++i) w[i] = c[i];
}

// words 0-7 of clip b's row: blocks 0-3 at idx = 4 b + j (both draw kernels)
__device__ __forceinline__ void aug_draw_row(int b, int H, int W, float p, const dcv_aug_limits& lim, uint64_t seed, uint64_t offset, int32_t (&o)[8]) {
    uint32_t w[4][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) aug_philox_block(4ull * (uint64_t)b + j, seed, offset, w[j]);
    const bool g_flip = (lim.mask & DCV_AUG_FLIP) && aug_u01(w[0][0]) <= p;
    const bool g_tr = (lim.mask & DCV_AUG_TRANSLATE) && aug_u01(w[0][2]) <= p;
    const bool g_cut = (lim.mask & DCV_AUG_CUTOUT) && aug_u01(w[1][2]) <= p;
    const bool g_col = (lim.mask & DCV_AUG_COLOUR) && aug_u01(w[2][2]) <= p;
    o[0] = (g_flip && (w[0][1] >> 31)) ? 1 : 0;
    o[1] = g_tr ? (int32_t)(w[1][0] % (uint32_t)(2 * lim.mx + 1)) - lim.mx : 0;
    o[2] = g_tr ? (int32_t)(w[1][1] % (uint32_t)(2 * lim.my + 1)) - lim.my : 0;
    o[3] = g_cut ? (int32_t)(w[2][0] % (uint32_t)H) - lim.size / 2 : 0;
    o[4] = g_cut ? (int32_t)(w[2][1] % (uint32_t)W) - lim.size / 2 : 0;
    o[5] = g_cut ? lim.size : 0;
    const float gain = aug_mul_add(2.f * lim.contrast, aug_u01(w[3][0]) - 0.5f, 1.f);
    const float bias = aug_mul(lim.brightness, aug_u01(w[3][1]) - 0.5f);
    o[6] = __builtin_bit_cast(int32_t, g_col ? gain : 1.f);
    o[7] = __builtin_bit_cast(int32_t, g_col ? bias : 0.f);
}

__global__ __launch_bounds__(256) void aug_draw_kernel(int32_t* __restrict__ table, int B, int H, int W, const int32_t* __restrict__ state, dcv_aug_limits lim,
                                                       uint64_t seed, uint64_t offset) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    int32_t o[8];
    aug_draw_row(b, H, W, __builtin_bit_cast(float, state[DCV_AUG_P]), lim, seed, offset, o);
#pragma unroll
    for (int i = 0; i < 8; ++i) table[(int64_t)b * 8 + i] = o[i];
}

// ---- interpolated warps and saturation: the (B, 24) row ---------------------------------------------------------------------------------
// The numpy restatement is tests/augwarp.py.  Every fp32 operation below is rounded on its own (contract(off) above); a unary minus of the specification is 0 - x.
struct AugWarpArgs {
    AugSrc src[2], frame, base;      // as in AugArgs
    float* y;
    int64_t osn, osc, osd, osh, osw;
    const int32_t* table;            // (B, 24)
    int32_t C, T, H, W;
    int32_t colour, vec, tf;
    int32_t tpw, tparts, wgs_per_clip;      // a workgroup owns 256 pixels of `tpw` frames (with all their channels) of one clip: wgs_per_clip = pixel blocks x tparts
    FastDiv div_w;
};

struct AugWarpRow {
    AugRow r;                        // words 0-7, as the exact path reads them
    bool warp, sat;
    float a, b, c, d, e, f, l00, l01, l10, l11, s, cx, cy;
};

static const int AUG_WARP_BOX = 9;       // the adjoint scans at most 9 x 9 output pixels per source pixel ...
// ... and keeps every one that taps it.  The hits are the lattice points of the parallelogram L (-1, 1)^2 about the centre; a convex region of area A and perimeter P
// holds at most A + P / 2 + 1 of them, and the draw's limits (sx, sy <= scale_max * aniso_max <= 2: a rectangle of sides 2 sx, 2 sy) give 16 + 8 + 1 = 25.  A
// hand-made row is in contract when 4 |det L| + 2 (|L e1| + |L e2|) + 1 <= 25 and its row sums fit the box; beyond that the first 25 hits count (memory-safe).
static const int AUG_WARP_HITS = 25;

__device__ __forceinline__ bool aug_finite(float v) { return __builtin_fabsf(v) < __builtin_inff(); }
// floor of a coordinate as an index, clamped before the conversion: every tap index is then within [-2, n + 1]
__device__ __forceinline__ int aug_index(float fl, int n) { return (int)fminf(fmaxf(fl, -2.f), (float)n); }

// The four taps of output pixel (h, w): the floors' indices and the weights, in tap order (y0,x0) (y0,x0+1) (y0+1,x0) (y0+1,x0+1).  FWD and BWD call this one function,
// so the adjoint sees the forward's bits.
struct AugTaps {
    int x0, y0;
    float w[4];
    bool ok;      // finite coordinates
};
__device__ __forceinline__ AugTaps aug_taps(const AugWarpRow& r, int h, int w, int H, int W) {
    const float u = (float)w - r.cx, v = (float)h - r.cy;
    const float su = (aug_mul(r.a, u) + aug_mul(r.b, v)) + r.c;
    const float sv = (aug_mul(r.d, u) + aug_mul(r.e, v)) + r.f;
    const float sx = su + r.cx, sy = sv + r.cy;
    AugTaps t;
    t.ok = aug_finite(sx) && aug_finite(sy);
    const float x0 = floorf(sx), y0 = floorf(sy);
    const float fx = sx - x0, fy = sy - y0;
    const float gx = 1.f - fx, gy = 1.f - fy;
    t.x0 = aug_index(x0, W); t.y0 = aug_index(y0, H);
    t.w[0] = aug_mul(gy, gx); t.w[1] = aug_mul(gy, fx); t.w[2] = aug_mul(fy, gx); t.w[3] = aug_mul(fy, fx);
    return t;
}

__device__ __forceinline__ float aug_third() { return __builtin_bit_cast(float, 0x3EAAAAABu); }
// the colour step on one source pixel's channels: saturation about the channel mean (C == 3 only), then gain and bias
__device__ __forceinline__ void aug_colour_fwd(float (&v)[3], int nc, const AugWarpRow& r) {
    if (r.sat) {
        const float m = aug_mul((v[0] + v[1]) + v[2], aug_third());
#pragma unroll
        for (int j = 0; j < 3; ++j) v[j] = m + aug_mul(r.s, v[j] - m);
    }
#pragma unroll
    for (int j = 0; j < 3; ++j)
        if (j < nc) v[j] = aug_mul_add(v[j], r.r.gain, r.r.bias);
}
// ... and its transpose on a gathered cotangent
__device__ __forceinline__ void aug_colour_bwd(float (&v)[3], int nc, const AugWarpRow& r) {
#pragma unroll
    for (int j = 0; j < 3; ++j)
        if (j < nc) v[j] = aug_mul(r.r.gain, v[j]);
    if (r.sat) {
        const float m = aug_mul((v[0] + v[1]) + v[2], aug_third());
#pragma unroll
        for (int j = 0; j < 3; ++j) v[j] = m + aug_mul(r.s, v[j] - m);
    }
}

// What a lane knows about its pixel before it walks the frames: computed once, reused across planes.
struct AugWarpGeo {
    int ih, iw;         // exact path: the one input pixel (clamped into the plane)
    bool inr, ok;       //   in range; in range and outside the cutout box
    AugTaps taps;       // FWD, interpolating
    bool tv[4], cut;    //   tap k is inside the plane and has a non-zero weight; the output pixel is inside the box
    int nhits, hlo, wlo;       // BWD, interpolating: the lane's hits — which candidates of the box at (hlo, wlo), as a bit per candidate (row-major, 9 per row) ...
    uint64_t hit_lo, hit_hi;   //   ... and their weights in LDS, in scan order
};

// One operand's term for channels c .. c + nc - 1 of one frame at the lane's pixel.  `p`: the operand at (b, c, t).
template <bool BWD>
__device__ __forceinline__ void aug_warp_term(const AugWarpArgs& a, const AugWarpRow& r, const AugWarpGeo& g, const AugSrc& s, const float* p, int c, int nc,
                                              const float (*hit_wt)[256], float (&term)[3]) {
    const bool mix = a.vec && nc == 2;
    float acc[3] = {0.f, 0.f, 0.f};
    if (!r.warp) {      // exact: bits move, as in aug_body
        if (g.inr) {
            const float* q = p + (int64_t)g.ih * s.sh + (int64_t)g.iw * s.sw;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                if (j >= nc) continue;
                uint32_t bits = __builtin_bit_cast(uint32_t, q[(int64_t)j * s.sc]);
                if (j == 0 && c == 0 && a.vec && r.r.flip) bits ^= 0x80000000u;
                acc[j] = __builtin_bit_cast(float, bits);
            }
        }
        if (a.colour) {
            if (BWD) aug_colour_bwd(acc, nc, r);
            else aug_colour_fwd(acc, nc, r);
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) term[j] = g.ok ? acc[j] : 0.f;
        return;
    }
    if (!BWD) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (!g.tv[k]) continue;
            const float* q = p + (int64_t)(g.taps.y0 + (k >> 1)) * s.sh + (int64_t)(g.taps.x0 + (k & 1)) * s.sw;
            float v[3] = {0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < 3; ++j)
                if (j < nc) v[j] = q[(int64_t)j * s.sc];
            if (a.colour) aug_colour_fwd(v, nc, r);
#pragma unroll
            for (int j = 0; j < 3; ++j) acc[j] = acc[j] + aug_mul(g.taps.w[k], v[j]);
        }
        if (mix) {      // a mirrored or rotated flow field's vectors turn with it
            const float r0 = acc[0], r1 = acc[1];
            acc[0] = aug_mul(r.l00, r0) + aug_mul(r.l01, r1);
            acc[1] = aug_mul(r.l10, r0) + aug_mul(r.l11, r1);
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) term[j] = g.cut ? 0.f : acc[j];
        return;
    }
    uint64_t lo = g.hit_lo, hi = g.hit_hi;
    for (int i = 0; i < g.nhits; ++i) {      // ascending bits: h ascending, then w ascending
        int idx;
        if (lo) { idx = __builtin_ctzll(lo); lo &= lo - 1; }
        else { idx = 64 + __builtin_ctzll(hi); hi &= hi - 1; }
        const int dh = (idx * 57) >> 9;      // idx / 9 for idx < 81
        const float wt = hit_wt[i][threadIdx.x];
        const float* q = p + (int64_t)(g.hlo + dh) * s.sh + (int64_t)(g.wlo + idx - dh * AUG_WARP_BOX) * s.sw;
        float v[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 3; ++j)
            if (j < nc) v[j] = q[(int64_t)j * s.sc];
        if (mix) {      // L^T on the cotangent
            const float d0 = v[0], d1 = v[1];
            v[0] = aug_mul(r.l00, d0) + aug_mul(r.l10, d1);
            v[1] = aug_mul(r.l01, d0) + aug_mul(r.l11, d1);
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) acc[j] = acc[j] + aug_mul(wt, v[j]);
    }
    if (a.colour) aug_colour_bwd(acc, nc, r);
#pragma unroll
    for (int j = 0; j < 3; ++j) term[j] = acc[j];
}

template <bool BWD>
__global__ __launch_bounds__(256) void aug_warp_kernel(AugWarpArgs a) {
    __shared__ float hit_wt[BWD ? AUG_WARP_HITS : 1][256];      // [hit][lane]: a lane's list is conflict-free (the forward's one row is unused and removed by the compiler)
    const int b = (int)(blockIdx.x / (uint32_t)a.wgs_per_clip);      // workgroup-uniform, so the row is scalar and the warp / exact branch uniform
    const int run = (int)blockIdx.x - b * a.wgs_per_clip;
    const int32_t* __restrict__ row = a.table + (int64_t)b * DCV_AUG_WARP_ROW_WORDS;
    const int H = a.H, W = a.W;
    AugWarpRow r;
    r.r.flip = row[0] != 0;
    const int dx = min(max(row[1], -W), W), dy = min(max(row[2], -H), H);
    r.r.cy0 = row[3]; r.r.cx0 = row[4];
    r.r.cy1 = r.r.cy0 + (int64_t)row[5]; r.r.cx1 = r.r.cx0 + (int64_t)row[5];
    r.r.gain = a.colour ? __builtin_bit_cast(float, row[6]) : 1.f;
    r.r.bias = a.colour ? __builtin_bit_cast(float, row[7]) : 0.f;
    r.r.s = r.r.flip ? -1 : 1;
    r.r.acol = r.r.flip ? W - 1 + dx : (BWD ? dx : -dx);
    r.r.rdy = BWD ? dy : -dy;
    r.r.aligned = false;
    r.warp = row[8] != 0;
    r.a = __builtin_bit_cast(float, row[9]); r.b = __builtin_bit_cast(float, row[10]); r.c = __builtin_bit_cast(float, row[11]);
    r.d = __builtin_bit_cast(float, row[12]); r.e = __builtin_bit_cast(float, row[13]); r.f = __builtin_bit_cast(float, row[14]);
    r.l00 = __builtin_bit_cast(float, row[15]); r.l01 = __builtin_bit_cast(float, row[16]);
    r.l10 = __builtin_bit_cast(float, row[17]); r.l11 = __builtin_bit_cast(float, row[18]);
    r.s = __builtin_bit_cast(float, row[19]);
    r.sat = a.colour && a.C == 3 && r.s != 1.f;      // s == 1 skips the step: m + (v - m) is not v in every bit
    r.cx = aug_mul((float)(W - 1), 0.5f); r.cy = aug_mul((float)(H - 1), 0.5f);
    const int blk = run / a.tparts, part = run - blk * a.tparts;
    const int t0 = part * a.tpw, t1 = min(t0 + a.tpw, a.T);
    // adjoint: half-extents of the box of outputs that can have a source pixel among their taps, |l00| + |l01| and |l10| + |l11| plus one pixel, capped
    const float ex = fminf((__builtin_fabsf(r.l00) + __builtin_fabsf(r.l01)) + 1.f, 4.f), ey = fminf((__builtin_fabsf(r.l10) + __builtin_fabsf(r.l11)) + 1.f, 4.f);
    const int px = blk * 256 + (int)threadIdx.x;      // one pixel per lane: its geometry (in the adjoint the candidate scan) is paid once for all the frames
    if (px < H * W) {
        const int oh = (int)fdiv((uint32_t)px, a.div_w), ow = px - oh * W;
        AugWarpGeo g;
        g.ih = g.iw = 0; g.inr = g.ok = g.cut = false; g.nhits = g.hlo = g.wlo = 0; g.hit_lo = g.hit_hi = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) g.tv[k] = false;
        if (!r.warp) {
            const int ih = oh + r.r.rdy, iw = r.r.acol + r.r.s * ow;
            g.inr = (unsigned)ih < (unsigned)H && (unsigned)iw < (unsigned)W;
            g.ih = g.inr ? ih : 0; g.iw = g.inr ? iw : 0;
            const int64_t ch = BWD ? ih : oh, cw = BWD ? iw : ow;
            g.ok = g.inr && !(ch >= r.r.cy0 && ch < r.r.cy1 && cw >= r.r.cx0 && cw < r.r.cx1);
        } else if (!BWD) {
            g.cut = oh >= r.r.cy0 && oh < r.r.cy1 && ow >= r.r.cx0 && ow < r.r.cx1;
            g.taps = aug_taps(r, oh, ow, H, W);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int ty = g.taps.y0 + (k >> 1), tx = g.taps.x0 + (k & 1);
                g.tv[k] = !g.cut && g.taps.ok && (unsigned)ty < (unsigned)H && (unsigned)tx < (unsigned)W && g.taps.w[k] != 0.f;
            }
        } else {
            // source pixel (oh, ow): scan h ascending, then w ascending, and keep the outputs that tap it
            const float du = ((float)ow - r.cx) - r.c, dv = ((float)oh - r.cy) - r.f;
            const float ocx = (aug_mul(r.l00, du) + aug_mul(r.l01, dv)) + r.cx, ocy = (aug_mul(r.l10, du) + aug_mul(r.l11, dv)) + r.cy;
            if (aug_finite(ocx) && aug_finite(ocy)) {
                const int wlo = (int)fminf(fmaxf(ceilf(ocx - ex), 0.f), (float)W), hlo = (int)fminf(fmaxf(ceilf(ocy - ey), 0.f), (float)H);
                const int whi = min((int)fminf(fmaxf(floorf(ocx + ex), -1.f), (float)(W - 1)), wlo + AUG_WARP_BOX - 1);
                const int hhi = min((int)fminf(fmaxf(floorf(ocy + ey), -1.f), (float)(H - 1)), hlo + AUG_WARP_BOX - 1);
                g.hlo = hlo; g.wlo = wlo;
                for (int h = hlo; h <= hhi; ++h)
                    for (int w = wlo; w <= whi; ++w) {
                        if (h >= r.r.cy0 && h < r.r.cy1 && w >= r.r.cx0 && w < r.r.cx1) continue;
                        const AugTaps t = aug_taps(r, h, w, H, W);
                        const int kx = ow - t.x0, ky = oh - t.y0;
                        if (!t.ok || (unsigned)kx > 1u || (unsigned)ky > 1u) continue;
                        const float wt = ky ? (kx ? t.w[3] : t.w[2]) : (kx ? t.w[1] : t.w[0]);
                        if (wt != 0.f && g.nhits < AUG_WARP_HITS) {
                            const int idx = (h - hlo) * AUG_WARP_BOX + (w - wlo);      // < 81: both extents are capped at 9
                            if (idx < 64) g.hit_lo |= 1ull << idx;
                            else g.hit_hi |= 1ull << (idx - 64);
                            hit_wt[g.nhits][threadIdx.x] = wt;
                            ++g.nhits;
                        }
                    }
            }
        }
        for (int t = t0; t < t1; ++t) {
            for (int c = 0; c < a.C;) {
                // the channels that need each other go together: a flow field's two components, a colour pixel's three under saturation
                const int nc = (c == 0 && a.vec) ? 2 : ((c == 0 && r.sat) ? 3 : 1);
                float o[3] = {0.f, 0.f, 0.f};
                bool have = false;
                if (BWD && a.base.on) {
                    const float* z = a.base.p + (int64_t)b * a.base.sn + (int64_t)c * a.base.sc + (int64_t)t * a.base.sd + (int64_t)oh * a.base.sh + (int64_t)ow * a.base.sw;
#pragma unroll
                    for (int j = 0; j < 3; ++j)
                        if (j < nc) o[j] = z[(int64_t)j * a.base.sc];
                    have = true;
                }
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const AugSrc& s = k < 2 ? a.src[k] : a.frame;
                    if (!s.on || (!BWD && k > 0) || (k == 2 && t != a.tf)) continue;      // workgroup-uniform
                    float term[3];
                    aug_warp_term<BWD>(a, r, g, s, s.p + (int64_t)b * s.sn + (int64_t)c * s.sc + (k == 2 ? 0 : (int64_t)t * s.sd), c, nc, hit_wt, term);
#pragma unroll
                    for (int j = 0; j < 3; ++j) o[j] = have ? o[j] + term[j] : term[j];      // the operands' order: base, src[0], src[1], frame
                    have = true;
                }
                float* yout = a.y + (int64_t)b * a.osn + (int64_t)c * a.osc + (int64_t)t * a.osd + (int64_t)oh * a.osh + (int64_t)ow * a.osw;
#pragma unroll
                for (int j = 0; j < 3; ++j)
                    if (j < nc) yout[(int64_t)j * a.osc] = have ? o[j] : 0.f;
                c += nc;
            }
        }
    }
}

static int aug_warp_launch(const char* who, bool bwd, const float* base, const dcv_dims5* based, const float* x, const dcv_dims5* xd, const float* x1,
                           const dcv_dims5* x1d, const float* xf, const dcv_dims5* xfd, int frame, const int32_t* table, int table_rows, float* y, const dcv_dims5* yd,
                           int colour, int vec, void* stream) {
    if (const int rc = aug_check(who, bwd, base, based, x, xd, x1, x1d, xf, xfd, frame, table, table_rows, y, yd)) return rc;
    const int64_t hw = (int64_t)yd->h * yd->w;
    if ((vec != 0 && vec != 1) || (vec && colour)) return fail(DCV_EINVAL, "%s: vector_channels is 0 or 1, and 0 on the colour stream (got %d, colour %d)", who, vec, colour);
    if (vec && yd->c < 2) return fail(DCV_EINVAL, "%s: vector_channels needs the field's two components, the clip has %d channel", who, yd->c);
    AugWarpArgs a;
    memset(&a, 0, sizeof(a));
    a.src[0] = aug_src(x, xd); a.src[1] = aug_src(x1, x1d); a.frame = aug_src(xf, xfd); a.base = aug_src(base, based);
    a.tf = frame;
    a.y = y; a.table = table;
    a.osn = yd->sn; a.osc = yd->sc; a.osd = yd->sd; a.osh = yd->sh; a.osw = yd->sw;
    a.C = yd->c; a.T = yd->d; a.H = yd->h; a.W = yd->w;
    a.colour = colour ? 1 : 0; a.vec = vec;
    // a workgroup keeps one clip (one row), 256 pixels and whole frames: saturation and the vector mix need a frame's channels together.  The frames are split
    // only as far as ~2048 workgroups need it: every split repeats the pixels' geometry
    const int64_t blocks = (hw + 255) / 256;
    int64_t tparts = 2048 / std::max<int64_t>((int64_t)yd->n * blocks, 1);
    tparts = std::min<int64_t>(std::max<int64_t>(tparts, 1), yd->d);
    const int64_t tpw = (yd->d + tparts - 1) / tparts;
    a.tpw = (int32_t)tpw;
    a.tparts = (int32_t)((yd->d + tpw - 1) / tpw);
    a.wgs_per_clip = (int32_t)(blocks * a.tparts);
    const int64_t grid = (int64_t)yd->n * a.wgs_per_clip;
    if (grid >= (1ll << 31)) return fail(DCV_EUNSUPPORTED, "%s: too many workgroups", who);
    a.div_w = make_fastdiv((uint32_t)yd->w);
    if (bwd) hipLaunchKernelGGL(aug_warp_kernel<true>, dim3((unsigned)grid), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    else hipLaunchKernelGGL(aug_warp_kernel<false>, dim3((unsigned)grid), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    DCV_LAUNCH_CHECK();
    return DCV_OK;
}

// The (B, 24) table: words 0-7 are aug_draw_row's; blocks 4-6 of clip b sit at idx = 4 B + 4 b + (j - 4).  + - * / only, so the numpy restatement is exact.
__device__ __forceinline__ float aug_vv(uint32_t w) { const float u = aug_u01(w); return (u + u) - 1.f; }
__device__ __forceinline__ float aug_ratio(uint32_t w, float m) {
    const float vv = aug_vv(w);
    const float k = aug_mul(m - 1.f, __builtin_fabsf(vv));
    return vv >= 0.f ? 1.f + k : 1.f / (1.f + k);
}

__global__ __launch_bounds__(256) void aug_warp_draw_kernel(int32_t* __restrict__ table, int B, int H, int W, const int32_t* __restrict__ state, dcv_aug_limits lim,
                                                            dcv_aug_warp_limits wl, uint64_t seed, uint64_t offset) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    const float p = __builtin_bit_cast(float, state[DCV_AUG_P]);
    int32_t o[DCV_AUG_WARP_ROW_WORDS];
    int32_t o8[8];
    aug_draw_row(b, H, W, p, lim, seed, offset, o8);
#pragma unroll
    for (int i = 0; i < 8; ++i) o[i] = o8[i];
    uint32_t w[3][4];
#pragma unroll
    for (int j = 0; j < 3; ++j) aug_philox_block(4ull * (uint64_t)B + 4ull * (uint64_t)b + j, seed, offset, w[j]);
    const bool g_scale = (wl.mask & DCV_AUG_SCALE) && aug_u01(w[0][0]) <= p;
    const bool g_rot = (wl.mask & DCV_AUG_ROTATE) && aug_u01(w[0][2]) <= p;
    const bool g_aniso = (wl.mask & DCV_AUG_ANISO) && aug_u01(w[1][0]) <= p;
    const bool g_sub = (wl.mask & DCV_AUG_SUBPIXEL) && aug_u01(w[1][2]) <= p;
    const bool g_sat = (wl.mask & DCV_AUG_SATURATION) && aug_u01(w[2][1]) <= p;
    const float s_iso = g_scale ? aug_ratio(w[0][1], wl.scale_max) : 1.f;
    float cs = 1.f, sn = 0.f;
    if (g_rot) {      // the half-angle tangent: cos and sin by + - * / alone
        const float t = aug_mul(wl.rot_tan_half, aug_vv(w[0][3]));
        const float tt = aug_mul(t, t), den = 1.f + tt;
        cs = (1.f - tt) / den; sn = (t + t) / den;
    }
    const float ra = g_aniso ? aug_ratio(w[1][1], wl.aniso_max) : 1.f;
    const float sx = aug_mul(s_iso, ra), sy = s_iso / ra;
    const float tx = g_sub ? aug_mul(aug_mul(wl.frac, (float)W), aug_vv(w[1][3])) : 0.f;
    const float ty = g_sub ? aug_mul(aug_mul(wl.frac, (float)H), aug_vv(w[2][0])) : 0.f;
    const float sat = g_sat ? 1.f + aug_mul(wl.sat, aug_vv(w[2][2])) : 1.f;
    const float phi = o[0] ? -1.f : 1.f;
    const float taux = (float)o[1] + tx, tauy = (float)o[2] + ty;
    const float l00 = aug_mul(aug_mul(cs, sx), phi), l01 = 0.f - aug_mul(sn, sy), l10 = aug_mul(aug_mul(sn, sx), phi), l11 = aug_mul(cs, sy);
    const float ia = aug_mul(phi, cs / sx), ib = aug_mul(phi, sn / sx), id = 0.f - sn / sy, ie = cs / sy;
    const float ic = 0.f - (aug_mul(ia, taux) + aug_mul(ib, tauy)), jf = 0.f - (aug_mul(id, taux) + aug_mul(ie, tauy));
    o[8] = (g_scale || g_rot || g_aniso || g_sub) ? 1 : 0;
    const float fw[11] = {ia, ib, ic, id, ie, jf, l00, l01, l10, l11, sat};
#pragma unroll
    for (int i = 0; i < 11; ++i) o[9 + i] = __builtin_bit_cast(int32_t, fw[i]);
#pragma unroll
    for (int i = 20; i < DCV_AUG_WARP_ROW_WORDS; ++i) o[i] = 0;
#pragma unroll
    for (int i = 0; i < DCV_AUG_WARP_ROW_WORDS; ++i) table[(int64_t)b * DCV_AUG_WARP_ROW_WORDS + i] = o[i];
}

// ---- the adaptive probability --------------------------------------------------------------------------------------------------------------------------
// One workgroup: integer sums, so the result does not depend on the order, and the order is fixed anyway.
__global__ __launch_bounds__(256) void aug_observe_kernel(const float* __restrict__ y, int n, int32_t* __restrict__ state) {
    __shared__ int32_t red[4];
    int32_t s = 0;
    for (int i = threadIdx.x; i < n; i += 256) {
        const float v = y[i];
        s += (v > 0.f) ? 1 : ((v < 0.f) ? -1 : 0);      // sign(0) = 0; a NaN compares false twice
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        state[DCV_AUG_SUM_SIGN] += red[0] + red[1] + red[2] + red[3];
        state[DCV_AUG_COUNT] += n;
    }
}

__global__ void aug_adjust_kernel(int32_t* __restrict__ state, double target, float step, float p_max) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int32_t sum = state[DCV_AUG_SUM_SIGN], count = state[DCV_AUG_COUNT];
    if (count > 0) {
        const double d = (double)sum / (double)count - target;
        const float sg = d > 0.0 ? 1.f : (d < 0.0 ? -1.f : 0.f);
        float p = __builtin_bit_cast(float, state[DCV_AUG_P]);
        p = fminf(fmaxf(p + sg * step, 0.f), p_max);      // sg * step is exact
        state[DCV_AUG_P] = __builtin_bit_cast(int32_t, p);
    }
    state[DCV_AUG_SUM_SIGN] = 0;
    state[DCV_AUG_COUNT] = 0;
    state[DCV_AUG_ADJUSTS] += 1;
}

}  // namespace dcv

using namespace dcv;

extern "C" {

int dcv_aug_apply(const float* x, const dcv_dims5* xd, const int32_t* table, int table_rows, float* y, const dcv_dims5* yd, int colour, int flip_negate_channel,
                  void* stream) {
    if (!x || !xd) return fail(DCV_EINVAL, "aug_apply: null argument");
    return aug_launch("aug_apply", false, nullptr, nullptr, x, xd, nullptr, nullptr, nullptr, nullptr, 0, table, table_rows, y, yd, colour, flip_negate_channel, stream);
}

int dcv_aug_apply_backward(const float* dy, const dcv_dims5* dyd, const int32_t* table, int table_rows, float* dx, const dcv_dims5* dxd, int colour,
                           int flip_negate_channel, void* stream) {
    if (!dy || !dyd) return fail(DCV_EINVAL, "aug_apply_backward: null argument");
    return aug_launch("aug_apply_backward", true, nullptr, nullptr, dy, dyd, nullptr, nullptr, nullptr, nullptr, 0, table, table_rows, dx, dxd, colour,
                      flip_negate_channel, stream);
}

int dcv_aug_fan_backward(const float* base, const dcv_dims5* based, const float* dy0, const dcv_dims5* dy0d, const float* dy1, const dcv_dims5* dy1d,
                         const float* dyf, const dcv_dims5* dyfd, int frame, const int32_t* table, int table_rows, float* dx, const dcv_dims5* dxd, int colour,
                         int flip_negate_channel, void* stream) {
    return aug_launch("aug_fan_backward", true, base, based, dy0, dy0d, dy1, dy1d, dyf, dyfd, frame, table, table_rows, dx, dxd, colour, flip_negate_channel, stream);
}

int dcv_aug_draw(int32_t* table, int B, int H, int W, const int32_t* state, const dcv_aug_limits* limits, uint64_t seed, uint64_t offset, void* stream) {
    if (!table || !state || !limits) return fail(DCV_EINVAL, "aug_draw: null argument");
    if (B < 1 || H < 1 || W < 1 || H > AUG_MAX_HW || W > AUG_MAX_HW) return fail(DCV_EINVAL, "aug_draw: bad B, H or W (%d, %d, %d)", B, H, W);
    const dcv_aug_limits& l = *limits;
    if (l.mx < 0 || l.my < 0 || l.size < 0 || l.mx > AUG_MAX_HW || l.my > AUG_MAX_HW || l.size > 2 * AUG_MAX_HW || (l.mask & ~15))
        return fail(DCV_EINVAL, "aug_draw: bad limits (mx %d, my %d, size %d, mask %d)", l.mx, l.my, l.size, l.mask);
    if (!(l.contrast >= 0.f) || !(l.brightness >= 0.f)) return fail(DCV_EINVAL, "aug_draw: contrast and brightness must be >= 0");
    hipLaunchKernelGGL(aug_draw_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), table, B, H, W, state, l, seed, offset);
    DCV_LAUNCH_CHECK();
    return DCV_OK;
}

int dcv_aug_warp_apply(const float* x, const dcv_dims5* xd, const int32_t* table, int table_rows, float* y, const dcv_dims5* yd, int colour, int vector_channels,
                       void* stream) {
    if (!x || !xd) return fail(DCV_EINVAL, "aug_warp_apply: null argument");
    return aug_warp_launch("aug_warp_apply", false, nullptr, nullptr, x, xd, nullptr, nullptr, nullptr, nullptr, 0, table, table_rows, y, yd, colour, vector_channels, stream);
}

int dcv_aug_warp_apply_backward(const float* dy, const dcv_dims5* dyd, const int32_t* table, int table_rows, float* dx, const dcv_dims5* dxd, int colour,
                                int vector_channels, void* stream) {
    if (!dy || !dyd) return fail(DCV_EINVAL, "aug_warp_apply_backward: null argument");
    return aug_warp_launch("aug_warp_apply_backward", true, nullptr, nullptr, dy, dyd, nullptr, nullptr, nullptr, nullptr, 0, table, table_rows, dx, dxd, colour,
                           vector_channels, stream);
}

int dcv_aug_warp_fan_backward(const float* base, const dcv_dims5* based, const float* dy0, const dcv_dims5* dy0d, const float* dy1, const dcv_dims5* dy1d,
                              const float* dyf, const dcv_dims5* dyfd, int frame, const int32_t* table, int table_rows, float* dx, const dcv_dims5* dxd, int colour,
                              int vector_channels, void* stream) {
    return aug_warp_launch("aug_warp_fan_backward", true, base, based, dy0, dy0d, dy1, dy1d, dyf, dyfd, frame, table, table_rows, dx, dxd, colour, vector_channels,
                           stream);
}

int dcv_aug_warp_draw(int32_t* table, int B, int H, int W, const int32_t* state, const dcv_aug_limits* limits, const dcv_aug_warp_limits* warp_limits, uint64_t seed,
                      uint64_t offset, void* stream) {
    if (!table || !state || !limits || !warp_limits) return fail(DCV_EINVAL, "aug_warp_draw: null argument");
    if (B < 1 || H < 1 || W < 1 || H > AUG_MAX_HW || W > AUG_MAX_HW) return fail(DCV_EINVAL, "aug_warp_draw: bad B, H or W (%d, %d, %d)", B, H, W);
    const dcv_aug_limits& l = *limits;
    if (l.mx < 0 || l.my < 0 || l.size < 0 || l.mx > AUG_MAX_HW || l.my > AUG_MAX_HW || l.size > 2 * AUG_MAX_HW || (l.mask & ~15))
        return fail(DCV_EINVAL, "aug_warp_draw: bad limits (mx %d, my %d, size %d, mask %d)", l.mx, l.my, l.size, l.mask);
    if (!(l.contrast >= 0.f) || !(l.brightness >= 0.f)) return fail(DCV_EINVAL, "aug_warp_draw: contrast and brightness must be >= 0");
    const dcv_aug_warp_limits& w = *warp_limits;
    const int32_t all = DCV_AUG_SCALE | DCV_AUG_ROTATE | DCV_AUG_ANISO | DCV_AUG_SUBPIXEL | DCV_AUG_SATURATION;
    // scale_max * aniso_max <= 2 and |theta| < 180 degrees keep |l00| + |l01| below 3: every drawn L is inside the adjoint's box
    if ((w.mask & ~all) || !(w.scale_max >= 1.f) || !(w.aniso_max >= 1.f) || !(w.scale_max * w.aniso_max <= 2.f) || !(w.rot_tan_half >= 0.f) ||
        !(w.rot_tan_half < __builtin_inff()) || !(w.frac >= 0.f && w.frac <= 1.f) || !(w.sat >= 0.f) || !(w.sat < __builtin_inff()))
        return fail(DCV_EINVAL, "aug_warp_draw: bad warp limits (mask %d, scale_max %g, aniso_max %g, rot_tan_half %g, frac %g, sat %g)", w.mask, w.scale_max,
                    w.aniso_max, w.rot_tan_half, w.frac, w.sat);
    hipLaunchKernelGGL(aug_warp_draw_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), table, B, H, W, state, l, w, seed, offset);
    DCV_LAUNCH_CHECK();
    return DCV_OK;
}

int dcv_aug_observe(const float* logits, int64_t n, int32_t* state, void* stream) {
    if (!logits || !state || n < 1 || n > (1 << 24)) return fail(DCV_EINVAL, "aug_observe: bad arguments (1 <= n <= 2^24)");
    hipLaunchKernelGGL(aug_observe_kernel, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream), logits, (int)n, state);
    DCV_LAUNCH_CHECK();
    return DCV_OK;
}

int dcv_aug_adjust(int32_t* state, double target, float step, float p_max, void* stream) {
    if (!state || !(step >= 0.f) || !(p_max >= 0.f && p_max <= 1.f) || !(target >= -1.0 && target <= 1.0)) return fail(DCV_EINVAL, "aug_adjust: bad arguments");
    hipLaunchKernelGGL(aug_adjust_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), state, target, step, p_max);
    DCV_LAUNCH_CHECK();
    return DCV_OK;
}

}  // extern "C"
