// HBM-bound kernels of the DCVGAN step for gfx950: BatchNorm (+Dropout2d +activation)
// forward/backward, activations, axpby / strided copy, Philox noise, GAN losses,
// GRU recurrence, Adam.  All work on NCDHW views: a "row" is one (n, c, d) plane
// of H*W contiguous floats (vectorised 16 B per lane); views whose (h, w) plane is
// not contiguous fall back to rows of one element.
#include "dcv_common.h"
#include <algorithm>
#include <vector>

namespace dcv {

extern thread_local char g_last_kernel[160];   // dcv_debug_last_kernel's text (conv_mfma.hip)

struct RowView {
    int64_t sn, sc, sd, sh, sw;
};

// rows = N*C*D*(H*W/inner); inner = contiguous run (H*W or 1)
struct RowMap {
    int32_t N, C, D, H, W;
    int32_t inner;   // contiguous run length in elements
    int32_t vec;     // 4 if inner % 4 == 0 and all views 16-B friendly, else 1
    int32_t gpr;     // groups (of vec elements) per row
    FastDiv div_gpr, div_cd, div_d, div_w;  // g -> row, row -> n, (c,d); tail -> (h,w) when inner == 1
    int64_t groups;
};

static bool plane_contig(const dcv_dims5& v) { return (v.w == 1 || v.sw == 1) && (v.h == 1 || v.sh == v.w); }

static RowMap make_rowmap(const dcv_dims5& shape, const dcv_dims5* const* views, int nviews, const void* const* ptrs) {
    RowMap m;
    memset(&m, 0, sizeof(m));
    m.N = shape.n; m.C = shape.c; m.D = shape.d; m.H = shape.h; m.W = shape.w;
    bool contig = true;
    for (int i = 0; i < nviews; ++i) contig = contig && plane_contig(*views[i]);
    const int hw = shape.h * shape.w;
    m.inner = contig ? hw : 1;
    bool v4 = contig && (hw % 4 == 0);
    if (v4)
        for (int i = 0; i < nviews; ++i) {
            const dcv_dims5& v = *views[i];
            if ((v.sn % 4) || (v.sc % 4) || (v.sd % 4) || (reinterpret_cast<uintptr_t>(ptrs[i]) % 16)) v4 = false;
        }
    m.vec = v4 ? 4 : 1;
    m.gpr = contig ? hw / m.vec : hw;  // when not contiguous: one group per element, "row" = (n,c,d)
    m.div_gpr = make_fastdiv((uint32_t)m.gpr);
    m.div_cd = make_fastdiv((uint32_t)(shape.c * shape.d));
    m.div_d = make_fastdiv((uint32_t)shape.d);
    m.div_w = make_fastdiv((uint32_t)shape.w);
    m.groups = (int64_t)shape.n * shape.c * shape.d * m.gpr;
    return m;
}

struct Pos {
    int n, c, d, col;  // col: element offset inside the (h, w) plane (first of the group)
    int h, w;
};

__device__ __forceinline__ Pos locate(const RowMap& m, uint32_t g) {
    Pos p;
    const uint32_t row = fdiv(g, m.div_gpr);
    const uint32_t cg = g - row * m.div_gpr.div;
    const uint32_t n = fdiv(row, m.div_cd);
    const uint32_t cd = row - n * m.div_cd.div;
    const uint32_t c = fdiv(cd, m.div_d);
    p.n = (int)n; p.c = (int)c; p.d = (int)(cd - c * m.div_d.div);
    p.col = (int)cg * m.vec;
    if (m.inner == 1) {
        const uint32_t h = fdiv(cg, m.div_w);
        p.h = (int)h; p.w = (int)(cg - h * m.div_w.div);
    } else {
        p.h = 0; p.w = 0;
    }
    return p;
}

__device__ __forceinline__ int64_t offs(const RowMap& m, const RowView& v, const Pos& p) {
    int64_t o = (int64_t)p.n * v.sn + (int64_t)p.c * v.sc + (int64_t)p.d * v.sd;
    if (m.inner == 1) o += (int64_t)p.h * v.sh + (int64_t)p.w * v.sw;
    else o += p.col;
    return o;
}

static RowView rv(const dcv_dims5& d) { return RowView{d.sn, d.sc, d.sd, d.sh, d.sw}; }

__device__ __forceinline__ float act_fwd(float v, int act, float slope) {
    if (act == DCV_ACT_LEAKY) return v > 0.f ? v : v * slope;
    if (act == DCV_ACT_TANH) return tanhf(v);
    return v;
}
// derivative evaluated from the OUTPUT y
__device__ __forceinline__ float act_bwd_from_y(float y, int act, float slope) {
    if (act == DCV_ACT_LEAKY) return y > 0.f ? 1.f : slope;
    if (act == DCV_ACT_TANH) return 1.f - y * y;
    return 1.f;
}

static inline unsigned grid_for(int64_t groups) {
    int64_t b = (groups + 255) / 256;
    if (b > 8192) b = 8192;   // 256 CUs x 8 blocks x 4: grid-stride beyond
    if (b < 1) b = 1;
    return (unsigned)b;
}

// ------------------------------------------------------------------------- //
// generic unary / binary elementwise kernels
// ------------------------------------------------------------------------- //
template <int VEC, class F>
__global__ __launch_bounds__(256) void ew_kernel(RowMap m, F f) {
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < m.groups; g += (int64_t)gridDim.x * 256) {
        const Pos p = locate(m, (uint32_t)g);
        f.template apply<VEC>(m, p);
    }
}

// Rows (one (n, c, d) plane = H * W contiguous floats) of at least 1024 floats: one workgroup per row.  Sample, channel and depth are
// then workgroup-uniform — the per-channel parameters arrive as scalar loads and the address is one scalar base plus the thread's
// column — instead of three magic divisions, 64-bit stride arithmetic and gathered parameter loads per 16 bytes of payload, which
// kept the generic kernel at 4.8 TB/s on a 1.17 GB activation where torch's plain elementwise kernel streams at 6.3.
template <class F>
__global__ __launch_bounds__(256) void ew_rows_kernel(RowMap m, F f) {
    const uint32_t row = blockIdx.x;
    Pos p;
    const uint32_t n = fdiv(row, m.div_cd);
    const uint32_t cd = row - n * m.div_cd.div;
    const uint32_t c = fdiv(cd, m.div_d);
    p.n = (int)n; p.c = (int)c; p.d = (int)(cd - c * m.div_d.div);
    p.h = 0; p.w = 0;
    for (int g = threadIdx.x; g < m.gpr; g += 256) {
        p.col = g * 4;
        f.template apply<4>(m, p);
    }
}

static bool ew_rows_off() {
    static const bool off = getenv("DCV_NO_EW_ROWS") != nullptr;
    return off;
}

// which kernel launch_ew takes for this map (the same conditions, for the BatchNorm entries' dcv_debug_last_kernel notes)
static bool ew_rows_ok(const RowMap& m) {
    return m.vec == 4 && m.inner != 1 && m.gpr % 256 == 0 && m.groups / m.gpr < (1ll << 31) && !ew_rows_off();
}
static const char* ew_name(const RowMap& m) { return m.groups == 0 ? "none" : ew_rows_ok(m) ? "ew_rows" : m.vec == 4 ? "ew<4>" : "ew<1>"; }

template <class F>
static int launch_ew(const RowMap& m, const F& f, hipStream_t s) {
    if (m.groups >= (1ll << 32)) return fail(DCV_EUNSUPPORTED, "elementwise: tensor too large");
    if (m.groups == 0) return DCV_OK;
    const int64_t rows = m.groups / m.gpr;
    if (ew_rows_ok(m))
        hipLaunchKernelGGL((ew_rows_kernel<F>), dim3((unsigned)rows), dim3(256), 0, s, m, f);
    else if (m.vec == 4) hipLaunchKernelGGL((ew_kernel<4, F>), dim3(grid_for(m.groups)), dim3(256), 0, s, m, f);
    else hipLaunchKernelGGL((ew_kernel<1, F>), dim3(grid_for(m.groups)), dim3(256), 0, s, m, f);
    DCV_LAUNCH_CHECK();
    return DCV_OK;
}

template <int VEC> struct Vec;
template <> struct Vec<4> { typedef float4 T; };
template <> struct Vec<1> { typedef float T; };
typedef float ew_f4 __attribute__((ext_vector_type(4)));
// DCV_EW_NT (A/B builds): non-temporal loads / stores in the streaming kernels (every byte is touched once per pass)
#ifdef DCV_EW_NT
#define DCV_EW_LD4(P) __builtin_nontemporal_load(reinterpret_cast<const ew_f4*>(P))
#define DCV_EW_ST4(P, V) __builtin_nontemporal_store((V), reinterpret_cast<ew_f4*>(P))
#else
#define DCV_EW_LD4(P) (*reinterpret_cast<const ew_f4*>(P))
#define DCV_EW_ST4(P, V) (*reinterpret_cast<ew_f4*>(P) = (V))
#endif
template <int VEC> __device__ __forceinline__ void ld(const float* p, float (&v)[VEC]) {
    if constexpr (VEC == 4) { const ew_f4 t = DCV_EW_LD4(p); v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3]; }
    else v[0] = *p;
}
template <int VEC> __device__ __forceinline__ void st(float* p, const float (&v)[VEC]) {
    if constexpr (VEC == 4) { const ew_f4 t = {v[0], v[1], v[2], v[3]}; DCV_EW_ST4(p, t); }
    else *p = v[0];
}

struct ActFwd {
    const float* x; float* y; RowView xv, yv; int act; float slope;
    template <int VEC> __device__ void apply(const RowMap& m, const Pos& p) const {
        float v[VEC];
        ld<VEC>(x + offs(m, xv, p), v);
#pragma unroll
        for (int i = 0; i < VEC; ++i) v[i] = act_fwd(v[i], act, slope);
        st<VEC>(y + offs(m, yv, p), v);
    }
};
struct ActBwd {
    const float* dy; const float* y; float* dx; RowView dyv, yv, dxv; int act; float slope;
    template <int VEC> __device__ void apply(const RowMap& m, const Pos& p) const {
        float g[VEC], o[VEC];
        ld<VEC>(dy + offs(m, dyv, p), g);
        ld<VEC>(y + offs(m, yv, p), o);
#pragma unroll
        for (int i = 0; i < VEC; ++i) g[i] *= act_bwd_from_y(o[i], act, slope);
        st<VEC>(dx + offs(m, dxv, p), g);
    }
};
struct Axpby {
    const float* x; const float* z; float* y; RowView xv, zv, yv; float a, b;
    template <int VEC> __device__ void apply(const RowMap& m, const Pos& p) const {
        float u[VEC];
        ld<VEC>(x + offs(m, xv, p), u);
        if (z) {
            float w[VEC];
            ld<VEC>(z + offs(m, zv, p), w);
#pragma unroll
            for (int i = 0; i < VEC; ++i) u[i] = a * u[i] + b * w[i];
        } else {
#pragma unroll
            for (int i = 0; i < VEC; ++i) u[i] = a * u[i];
        }
        st<VEC>(y + offs(m, yv, p), u);
    }
};

// ------------------------------------------------------------------------- //
// Philox4x32-10 + Box-Muller
// ------------------------------------------------------------------------- //
// (philox4x32_10 itself is in dcv_common.h: augment.hip draws with the same function)
// 4 N(0,1) samples for 128-bit counter (idx, stream offset)
__device__ __forceinline__ void normal4(uint64_t seed, uint64_t offset, uint64_t idx, float (&o)[4]) {
    uint32_t c[4] = {(uint32_t)idx, (uint32_t)(idx >> 32), (uint32_t)offset, (uint32_t)(offset >> 32)};
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    const float s = 2.3283064365386963e-10f;  // 2^-32
    const float u0 = ((float)c[0] + 0.5f) * s, u1 = ((float)c[1] + 0.5f) * s;
    const float u2 = ((float)c[2] + 0.5f) * s, u3 = ((float)c[3] + 0.5f) * s;
    const float r0 = sqrtf(-2.f * __logf(fmaxf(u0, 1e-30f))), r1 = sqrtf(-2.f * __logf(fmaxf(u2, 1e-30f)));
    float s0, c0, s1, c1;
    __sincosf(6.283185307179586f * u1, &s0, &c0);
    __sincosf(6.283185307179586f * u3, &s1, &c1);
    o[0] = r0 * c0; o[1] = r0 * s0; o[2] = r1 * c1; o[3] = r1 * s1;
}

struct NoiseAdd {
    const float* x; float* y; RowView xv, yv; float sigma; uint64_t seed, offset;
    template <int VEC> __device__ void apply(const RowMap& m, const Pos& p) const {
        float u[VEC];
        ld<VEC>(x + offs(m, xv, p), u);
        // logical (contiguous) element index -> counter; independent of the views' strides
        const uint64_t row = ((uint64_t)p.n * m.C + p.c) * m.D + p.d;
        const uint64_t e = row * ((uint64_t)m.H * m.W) + (m.inner == 1 ? (uint64_t)p.h * m.W + p.w : (uint64_t)p.col);
        float z[4];
        normal4(seed, offset, e >> 2, z);
        if constexpr (VEC == 4) {
#pragma unroll
            for (int i = 0; i < 4; ++i) u[i] += sigma * z[i];
        } else {
            u[0] += sigma * z[e & 3];
        }
        st<VEC>(y + offs(m, yv, p), u);
    }
};

__global__ void normal_fill_kernel(float* __restrict__ out, int64_t n, uint64_t seed, uint64_t offset) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q * 4 >= n) return;
    float z[4];
    normal4(seed, offset, (uint64_t)q, z);
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (q * 4 + i < n) out[q * 4 + i] = z[i];
}

// `count` consecutive draws of n values each in one launch: draw j is normal_fill_kernel's output for offset + j (the generator's per-frame motion noise: 16 launches of 5 000
// values each were 16 dependent launch latencies at the start of every generator pass)
__global__ void normal_fill_many_kernel(float* __restrict__ out, int64_t n, int64_t count, uint64_t seed, uint64_t offset) {
    const int64_t qpd = (n + 3) / 4, t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= qpd * count) return;
    const int64_t j = t / qpd, q = t - j * qpd;
    float z[4];
    normal4(seed, offset + (uint64_t)j, (uint64_t)q, z);
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (q * 4 + i < n) out[j * n + q * 4 + i] = z[i];
}

__global__ void dropout_mask_kernel(float* __restrict__ mask, int64_t n, float p, uint64_t seed, uint64_t offset) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q * 4 >= n) return;
    uint32_t c[4] = {(uint32_t)q, (uint32_t)((uint64_t)q >> 32), (uint32_t)offset, (uint32_t)(offset >> 32)};
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    const float keep = 1.f / (1.f - p);
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (q * 4 + i < n) mask[q * 4 + i] = (((float)c[i] + 0.5f) * 2.3283064365386963e-10f >= p) ? keep : 0.f;
}

// ------------------------------------------------------------------------- //
// BatchNorm
// ------------------------------------------------------------------------- //
// wave64 sum via DPP-free shuffles, then LDS across the 4 waves
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

template <int NV>
__device__ __forceinline__ void block_sum(double (&v)[NV], double* red /* [4][NV] */) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = wave_sum(v[i]);
    __syncthreads();
    if (lane == 0)
#pragma unroll
        for (int i = 0; i < NV; ++i) red[wave * NV + i] = v[i];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = red[i] + red[NV + i] + red[2 * NV + i] + red[3 * NV + i];
}

// channel-wise iteration: groups of channel c are g = (n*D + d)*gpr + cg
struct ChanMap {
    int32_t N, C, D, H, W, inner, vec, gpr;
    FastDiv div_gpr, div_d, div_w;
    int64_t per_chan;   // groups per channel
    int32_t split;      // blocks per channel
    int64_t seg;        // groups per block
};
static ChanMap make_chanmap(const RowMap& m) {
    ChanMap c;
    memset(&c, 0, sizeof(c));
    c.N = m.N; c.C = m.C; c.D = m.D; c.H = m.H; c.W = m.W; c.inner = m.inner; c.vec = m.vec; c.gpr = m.gpr;
    c.div_gpr = m.div_gpr; c.div_d = m.div_d; c.div_w = m.div_w;
    c.per_chan = (int64_t)m.N * m.D * m.gpr;
    int64_t split = (2048 + m.C - 1) / m.C;           // ~2048 blocks in total
    const int64_t maxsplit = (c.per_chan + 1023) / 1024;  // >= 4 groups per thread
    if (split > maxsplit) split = maxsplit;
    if (split < 1) split = 1;
    c.split = (int)split;
    c.seg = (c.per_chan + split - 1) / split;
    return c;
}
__device__ __forceinline__ Pos locate_c(const ChanMap& m, int c, uint32_t g) {
    Pos p;
    const uint32_t nd = fdiv(g, m.div_gpr);
    const uint32_t cg = g - nd * m.div_gpr.div;
    const uint32_t n = fdiv(nd, m.div_d);
    p.n = (int)n; p.c = c; p.d = (int)(nd - n * m.div_d.div);
    p.col = (int)cg * m.vec;
    if (m.inner == 1) {
        const uint32_t h = fdiv(cg, m.div_w);
        p.h = (int)h; p.w = (int)(cg - h * m.div_w.div);
    } else { p.h = 0; p.w = 0; }
    return p;
}
__device__ __forceinline__ int64_t offs_c(const ChanMap& m, const RowView& v, const Pos& p) {
    int64_t o = (int64_t)p.n * v.sn + (int64_t)p.c * v.sc + (int64_t)p.d * v.sd;
    if (m.inner == 1) o += (int64_t)p.h * v.sh + (int64_t)p.w * v.sw;
    else o += p.col;
    return o;
}

// partial[c][s] = {sum x, sum x^2} over the block's segment
template <int VEC>
__global__ __launch_bounds__(256) void bn_stats_kernel(ChanMap m, const float* __restrict__ x, RowView xv, double* __restrict__ partial) {
    __shared__ double red[8];
    const int c = blockIdx.x / m.split, s = blockIdx.x % m.split;
    const int64_t g0 = (int64_t)s * m.seg;
    int64_t g1 = g0 + m.seg;
    if (g1 > m.per_chan) g1 = m.per_chan;
    float a0 = 0.f, a1 = 0.f;
    double acc[2] = {0.0, 0.0};
    int cnt = 0;
    for (int64_t g = g0 + threadIdx.x; g < g1; g += 256) {
        const Pos p = locate_c(m, c, (uint32_t)g);
        float v[VEC];
        ld<VEC>(x + offs_c(m, xv, p), v);
#pragma unroll
        for (int i = 0; i < VEC; ++i) { a0 += v[i]; a1 += v[i] * v[i]; }
        if (++cnt == 64) { acc[0] += a0; acc[1] += a1; a0 = a1 = 0.f; cnt = 0; }  // bound fp32 run length
    }
    acc[0] += a0; acc[1] += a1;
    block_sum<2>(acc, red);
    if (threadIdx.x == 0) { partial[(int64_t)blockIdx.x * 2] = acc[0]; partial[(int64_t)blockIdx.x * 2 + 1] = acc[1]; }
}

__device__ __forceinline__ void bn_finalize_channel(int c, double s0, double s1, double count, float eps, float momentum,
                                                    float* __restrict__ save_mean, float* __restrict__ save_invstd,
                                                    float* __restrict__ running_mean, float* __restrict__ running_var) {
    const double mean = s0 / count;
    double var = s1 / count - mean * mean;
    if (var < 0) var = 0;
    save_mean[c] = (float)mean;
    save_invstd[c] = (float)(1.0 / sqrt(var + (double)eps));
    if (running_mean) {
        const double unbiased = count > 1 ? var * count / (count - 1) : var;
        running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * (float)mean;
        running_var[c] = (1.f - momentum) * running_var[c] + momentum * (float)unbiased;
    }
}

// `nbt`: the module's num_batches_tracked buffer (int64, may be NULL), bumped here instead of by a launch of its own
__global__ void bn_finalize_kernel(const double* __restrict__ partial, int C, int split, double count, float eps, float momentum,
                                   float* __restrict__ save_mean, float* __restrict__ save_invstd,
                                   float* __restrict__ running_mean, float* __restrict__ running_var, int64_t* __restrict__ nbt) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c == 0 && nbt) *nbt += 1;
    if (c >= C) return;
    double s0 = 0, s1 = 0;
    for (int k = 0; k < split; ++k) { s0 += partial[((int64_t)c * split + k) * 2]; s1 += partial[((int64_t)c * split + k) * 2 + 1]; }
    bn_finalize_channel(c, s0, s1, count, eps, momentum, save_mean, save_invstd, running_mean, running_var);
}

// conv -> BatchNorm pairs: {sum, sum^2} in fp64 from the conv epilogue's per-tile fp32 sums stat[part][pitch][2], finalised
// in the same launch (one block per channel)
__global__ __launch_bounds__(256) void bn_partials_finalize_kernel(const float* __restrict__ stat, int nparts, int pitch, double count, float eps, float momentum,
                                                                   float* __restrict__ save_mean, float* __restrict__ save_invstd,
                                                                   float* __restrict__ running_mean, float* __restrict__ running_var, int64_t* __restrict__ nbt) {
    __shared__ double red[8];
    const int c = blockIdx.x;
    double acc[2] = {0.0, 0.0};
    for (int p = threadIdx.x; p < nparts; p += 256) {
        const float2 v = *reinterpret_cast<const float2*>(stat + ((int64_t)p * pitch + c) * 2);
        acc[0] += (double)v.x;
        acc[1] += (double)v.y;
    }
    block_sum<2>(acc, red);
    if (threadIdx.x == 0) {
        if (c == 0 && nbt) *nbt += 1;
        bn_finalize_channel(c, acc[0], acc[1], count, eps, momentum, save_mean, save_invstd, running_mean, running_var);
    }
}

__global__ void bn_eval_stats_kernel(int C, float eps, const float* __restrict__ rm, const float* __restrict__ rv_, float* __restrict__ mean, float* __restrict__ invstd) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    mean[c] = rm[c];
    invstd[c] = 1.f / sqrtf(rv_[c] + eps);
}

struct BnApply {
    const float* x; float* y; RowView xv, yv;
    const float* gamma; const float* beta; const float* mean; const float* invstd; const float* mask;
    int act; float slope;
    template <int VEC> __device__ void apply(const RowMap& m, const Pos& p) const {
        float v[VEC];
        ld<VEC>(x + offs(m, xv, p), v);
        const float sc = gamma[p.c] * invstd[p.c];
        const float sh = beta[p.c] - mean[p.c] * sc;
        const float mk = mask ? mask[(int64_t)p.n * m.C + p.c] : 1.f;
#pragma unroll
        for (int i = 0; i < VEC; ++i) v[i] = act_fwd((v[i] * sc + sh) * mk, act, slope);
        st<VEC>(y + offs(m, yv, p), v);
    }
};

// backward pass 1: partial[c][s] = {sum dz, sum dz * xhat},  dz = dy * act'(z) * mask
template <int VEC>
__global__ __launch_bounds__(256) void bn_bwd_reduce_kernel(ChanMap m, const float* __restrict__ dy, RowView dyv, const float* __restrict__ x, RowView xv,
                                                            const float* __restrict__ gamma, const float* __restrict__ beta,
                                                            const float* __restrict__ mean, const float* __restrict__ invstd, const float* __restrict__ mask,
                                                            int act, float slope, double* __restrict__ partial) {
    __shared__ double red[8];
    const int c = blockIdx.x / m.split, s = blockIdx.x % m.split;
    const int64_t g0 = (int64_t)s * m.seg;
    int64_t g1 = g0 + m.seg;
    if (g1 > m.per_chan) g1 = m.per_chan;
    const float mu = mean[c], is = invstd[c], ga = gamma[c], be = beta[c];
    // the activation's branch is decided by EXACTLY the expression the forward pass evaluated (BnApply): a
    // pre-activation within rounding of zero must not come out positive there and non-positive here
    const float sc = ga * is, sh = be - mu * sc;
    float a0 = 0.f, a1 = 0.f;
    double acc[2] = {0.0, 0.0};
    int cnt = 0;
    for (int64_t g = g0 + threadIdx.x; g < g1; g += 256) {
        const Pos p = locate_c(m, c, (uint32_t)g);
        float v[VEC], d[VEC];
        ld<VEC>(x + offs_c(m, xv, p), v);
        ld<VEC>(dy + offs_c(m, dyv, p), d);
        const float mk = mask ? mask[(int64_t)p.n * m.C + c] : 1.f;
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            const float xh = (v[i] - mu) * is;
            const float z = (v[i] * sc + sh) * mk;
            float dz = d[i] * mk;
            if (act == DCV_ACT_LEAKY) dz *= (z > 0.f ? 1.f : slope);
            else if (act == DCV_ACT_TANH) { const float t = tanhf(z); dz *= 1.f - t * t; }
            a0 += dz; a1 += dz * xh;
        }
        if (++cnt == 64) { acc[0] += a0; acc[1] += a1; a0 = a1 = 0.f; cnt = 0; }
    }
    acc[0] += a0; acc[1] += a1;
    block_sum<2>(acc, red);
    if (threadIdx.x == 0) { partial[(int64_t)blockIdx.x * 2] = acc[0]; partial[(int64_t)blockIdx.x * 2 + 1] = acc[1]; }
}

// The same sums for planes of at least 1024 contiguous floats: a workgroup takes whole (n, d) rows of its channel, so the row's base
// addresses are scalar and the inner loop is two 16-byte loads per thread and trip with nothing else to compute (the generic kernel
// decodes every group with three magic divisions); the trips of a row are unrolled, which puts up to eight loads in flight per thread.
__global__ __launch_bounds__(256) void bn_bwd_reduce_rows_kernel(ChanMap m, const float* __restrict__ dy, RowView dyv, const float* __restrict__ x, RowView xv,
                                                                 const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                 const float* __restrict__ mean, const float* __restrict__ invstd, const float* __restrict__ mask,
                                                                 int act, float slope, double* __restrict__ partial) {
    __shared__ double red[8];
    const int c = blockIdx.x / m.split, s = blockIdx.x % m.split;
    const int rows = m.N * m.D, rps = (rows + m.split - 1) / m.split;
    const int r0 = s * rps, r1 = min(rows, r0 + rps);
    const float mu = mean[c], is = invstd[c], ga = gamma[c], be = beta[c];
    const float sc = ga * is, sh = be - mu * sc;   // the forward pass's expression decides the activation's branch (see above)
    float a0 = 0.f, a1 = 0.f;
    double acc[2] = {0.0, 0.0};
    int cnt = 0;
    for (int row = r0; row < r1; ++row) {
        const uint32_t n = fdiv((uint32_t)row, m.div_d);
        const int d = row - (int)n * m.D;
        const float* __restrict__ xr = x + (int64_t)n * xv.sn + (int64_t)c * xv.sc + (int64_t)d * xv.sd + 4 * threadIdx.x;
        const float* __restrict__ dr = dy + (int64_t)n * dyv.sn + (int64_t)c * dyv.sc + (int64_t)d * dyv.sd + 4 * threadIdx.x;
        const float mk = mask ? mask[(int64_t)n * m.C + c] : 1.f;
#pragma unroll 4
        for (int g = 0; g < m.gpr; g += 256) {
            const ew_f4 v = DCV_EW_LD4(xr + 4 * g);
            const ew_f4 dd = DCV_EW_LD4(dr + 4 * g);
            const float vv[4] = {v[0], v[1], v[2], v[3]}, dv[4] = {dd[0], dd[1], dd[2], dd[3]};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float xh = (vv[i] - mu) * is;
                const float z = (vv[i] * sc + sh) * mk;
                float dz = dv[i] * mk;
                if (act == DCV_ACT_LEAKY) dz *= (z > 0.f ? 1.f : slope);
                else if (act == DCV_ACT_TANH) { const float t = tanhf(z); dz *= 1.f - t * t; }
                a0 += dz; a1 += dz * xh;
            }
        }
        cnt += m.gpr >> 8;
        if (cnt >= 64) { acc[0] += a0; acc[1] += a1; a0 = a1 = 0.f; cnt = 0; }   // bound the fp32 run length (between rows: the trips stay branch-free)
    }
    acc[0] += a0; acc[1] += a1;
    block_sum<2>(acc, red);
    if (threadIdx.x == 0) { partial[(int64_t)blockIdx.x * 2] = acc[0]; partial[(int64_t)blockIdx.x * 2 + 1] = acc[1]; }
}

// dbeta = sum dz, dgamma = sum dz*xhat; coef[c] = {dbeta/count, dgamma/count} for pass 2
__global__ void bn_bwd_finalize_kernel(const double* __restrict__ partial, int C, int split, double count,
                                       float* __restrict__ dgamma, float* __restrict__ dbeta, float* __restrict__ coef) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    double s0 = 0, s1 = 0;
    for (int k = 0; k < split; ++k) { s0 += partial[((int64_t)c * split + k) * 2]; s1 += partial[((int64_t)c * split + k) * 2 + 1]; }
    dbeta[c] = (float)s0;
    dgamma[c] = (float)s1;
    coef[2 * c] = (float)(s0 / count);
    coef[2 * c + 1] = (float)(s1 / count);
}

struct BnBwdApply {
    const float* dy; const float* x; float* dx; RowView dyv, xv, dxv;
    const float* gamma; const float* beta; const float* mean; const float* invstd; const float* mask; const float* coef;
    int act; float slope; int training;
    template <int VEC> __device__ void apply(const RowMap& m, const Pos& p) const {
        float v[VEC], d[VEC];
        ld<VEC>(x + offs(m, xv, p), v);
        ld<VEC>(dy + offs(m, dyv, p), d);
        const int c = p.c;
        const float mu = mean[c], is = invstd[c], ga = gamma[c], be = beta[c];
        const float mk = mask ? mask[(int64_t)p.n * m.C + c] : 1.f;
        const float k0 = training ? coef[2 * c] : 0.f, k1 = training ? coef[2 * c + 1] : 0.f;
        const float sc = ga * is, sh = be - mu * sc;   // as in BnApply: same branch of the activation as the forward pass
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            const float xh = (v[i] - mu) * is;
            const float z = (v[i] * sc + sh) * mk;
            float dz = d[i] * mk;
            if (act == DCV_ACT_LEAKY) dz *= (z > 0.f ? 1.f : slope);
            else if (act == DCV_ACT_TANH) { const float t = tanhf(z); dz *= 1.f - t * t; }
            v[i] = ga * is * (dz - k0 - xh * k1);
        }
        st<VEC>(dx + offs(m, dxv, p), v);
    }
};

// ------------------------------------------------------------------------- //
// Small BatchNorm layers, one launch per pass (round 3).  The 4x4 / 2x2 / 1x1-spatial layers of the generators and the
// discriminators' trunks hold <= 32 K elements per channel: their passes are latency-bound ~5-25 us launches (statistics or
// partials-finalize + apply forward; reduce + finalize + apply backward: 40 + 40 + 53 launches per iteration, ~3 ms of kernel
// time).  Here ONE workgroup of 1024 threads owns a channel, keeps its elements in registers (<= 8 groups of 4 per thread and
// tensor), reduces over the workgroup in a fixed order (fp32 per thread over <= 32 terms, fp64 across lanes and waves),
// and applies — each tensor is read once and the pass is one launch.  Same expressions as the large-tensor kernels, so the
// (Leaky)ReLU branch decided in the backward pass is the forward pass's.
// ------------------------------------------------------------------------- //
constexpr int SMALL_NT = 1024, SMALL_K = 8;

__device__ __forceinline__ void block_sum_1024(double (&v)[2], double* red /* [16][2] */) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    v[0] = wave_sum(v[0]); v[1] = wave_sum(v[1]);
    __syncthreads();
    if (lane == 0) { red[wave * 2] = v[0]; red[wave * 2 + 1] = v[1]; }
    __syncthreads();
    double a = 0.0, b = 0.0;
#pragma unroll
    for (int w = 0; w < SMALL_NT / 64; ++w) { a += red[w * 2]; b += red[w * 2 + 1]; }
    v[0] = a; v[1] = b;
}

__global__ __launch_bounds__(SMALL_NT) void bn_fwd_small_kernel(ChanMap m, const float* __restrict__ x, RowView xv, float* __restrict__ y, RowView yv,
                                                                const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                float* __restrict__ running_mean, float* __restrict__ running_var, int64_t* __restrict__ nbt,
                                                                float* __restrict__ save_mean, float* __restrict__ save_invstd, const float* __restrict__ mask,
                                                                double count, float eps, float momentum, int act, float slope) {
    __shared__ double red[2 * SMALL_NT / 64];
    const int c = blockIdx.x;
    float4 v[SMALL_K];
    int32_t oy[SMALL_K];
    float mk[SMALL_K];
    float a0 = 0.f, a1 = 0.f;
#pragma unroll
    for (int k = 0; k < SMALL_K; ++k) {
        const int64_t g = (int64_t)threadIdx.x + (int64_t)k * SMALL_NT;
        v[k] = make_float4(0.f, 0.f, 0.f, 0.f); oy[k] = -1; mk[k] = 1.f;
        if (g < m.per_chan) {
            const Pos p = locate_c(m, c, (uint32_t)g);
            v[k] = *reinterpret_cast<const float4*>(x + offs_c(m, xv, p));
            oy[k] = (int32_t)offs_c(m, yv, p);
            if (mask) mk[k] = mask[(int64_t)p.n * m.C + c];
            a0 += (v[k].x + v[k].y) + (v[k].z + v[k].w);
            a1 += (v[k].x * v[k].x + v[k].y * v[k].y) + (v[k].z * v[k].z + v[k].w * v[k].w);
        }
    }
    double acc[2] = {(double)a0, (double)a1};
    block_sum_1024(acc, red);
    const double mean_d = acc[0] / count;
    double var = acc[1] / count - mean_d * mean_d;
    if (var < 0) var = 0;
    const float mu = (float)mean_d, is = (float)(1.0 / sqrt(var + (double)eps));
    if (threadIdx.x == 0) {
        if (c == 0 && nbt) *nbt += 1;
        bn_finalize_channel(c, acc[0], acc[1], count, eps, momentum, save_mean, save_invstd, running_mean, running_var);
    }
    const float sc = gamma[c] * is, sh = beta[c] - mu * sc;      // BnApply's expressions
#pragma unroll
    for (int k = 0; k < SMALL_K; ++k)
        if (oy[k] >= 0) {
            float4 o;
            o.x = act_fwd((v[k].x * sc + sh) * mk[k], act, slope);
            o.y = act_fwd((v[k].y * sc + sh) * mk[k], act, slope);
            o.z = act_fwd((v[k].z * sc + sh) * mk[k], act, slope);
            o.w = act_fwd((v[k].w * sc + sh) * mk[k], act, slope);
            *reinterpret_cast<float4*>(y + oy[k]) = o;
        }
}

__global__ __launch_bounds__(SMALL_NT) void bn_bwd_small_kernel(ChanMap m, const float* __restrict__ dy, RowView dyv, const float* __restrict__ x, RowView xv,
                                                                float* __restrict__ dx, RowView dxv, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                const float* __restrict__ mean, const float* __restrict__ invstd, const float* __restrict__ mask,
                                                                double count, int act, float slope, int training, float* __restrict__ dgamma, float* __restrict__ dbeta) {
    __shared__ double red[2 * SMALL_NT / 64];
    const int c = blockIdx.x;
    const float mu = mean[c], is = invstd[c], ga = gamma[c], be = beta[c];
    const float sc = ga * is, sh = be - mu * sc;                 // the forward pass's expression decides the activation's branch
    float4 dz[SMALL_K], xh[SMALL_K];
    int32_t od[SMALL_K];   // element offsets: these tensors are far below 2^31 elements (bn_small_ok)
    float a0 = 0.f, a1 = 0.f;
#pragma unroll
    for (int k = 0; k < SMALL_K; ++k) {
        const int64_t g = (int64_t)threadIdx.x + (int64_t)k * SMALL_NT;
        od[k] = -1;
        dz[k] = make_float4(0.f, 0.f, 0.f, 0.f); xh[k] = dz[k];
        if (g < m.per_chan) {
            const Pos p = locate_c(m, c, (uint32_t)g);
            const float4 v = *reinterpret_cast<const float4*>(x + offs_c(m, xv, p));
            const float4 d = *reinterpret_cast<const float4*>(dy + offs_c(m, dyv, p));
            od[k] = (int32_t)offs_c(m, dxv, p);
            const float mk = mask ? mask[(int64_t)p.n * m.C + c] : 1.f;
            const float vv[4] = {v.x, v.y, v.z, v.w}, dd[4] = {d.x, d.y, d.z, d.w};
            float zz[4], hh[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                hh[i] = (vv[i] - mu) * is;
                const float z = (vv[i] * sc + sh) * mk;
                float t = dd[i] * mk;
                if (act == DCV_ACT_LEAKY) t *= (z > 0.f ? 1.f : slope);
                else if (act == DCV_ACT_TANH) { const float th = tanhf(z); t *= 1.f - th * th; }
                zz[i] = t;
                a0 += t; a1 += t * hh[i];
            }
            dz[k] = make_float4(zz[0], zz[1], zz[2], zz[3]);
            xh[k] = make_float4(hh[0], hh[1], hh[2], hh[3]);
        }
    }
    double acc[2] = {(double)a0, (double)a1};
    block_sum_1024(acc, red);
    if (threadIdx.x == 0) { dbeta[c] = (float)acc[0]; dgamma[c] = (float)acc[1]; }
    const float k0 = training ? (float)(acc[0] / count) : 0.f, k1 = training ? (float)(acc[1] / count) : 0.f;   // bn_bwd_finalize_kernel's coef
#pragma unroll
    for (int k = 0; k < SMALL_K; ++k)
        if (od[k] >= 0) {
            float4 o;
            o.x = ga * is * (dz[k].x - k0 - xh[k].x * k1);
            o.y = ga * is * (dz[k].y - k0 - xh[k].y * k1);
            o.z = ga * is * (dz[k].z - k0 - xh[k].z * k1);
            o.w = ga * is * (dz[k].w - k0 - xh[k].w * k1);
            *reinterpret_cast<float4*>(dx + od[k]) = o;
        }
}

static bool bn_small_ok(const RowMap& m, const ChanMap& cm) {
    static const bool off = getenv("DCV_NO_BN_SMALL") != nullptr;
    return !off && m.vec == 4 && m.inner != 1 && cm.per_chan <= (int64_t)SMALL_NT * SMALL_K && cm.per_chan >= 64 && m.C >= 32 && m.groups < (1ll << 28);
}

// ------------------------------------------------------------------------- //
// Synchronised BatchNorm (data parallel, fp32 path).  The statistics and the backward's two sums cover the batch of ALL ranks: each rank
// leaves its own fp64 sums in a "row" of 2C + 1 doubles ({s0[c]}, {s1[c]}, count), the rows of all ranks are exchanged by the caller
// (one collective per BatchNorm group and pass), and every rank then adds the same table in rank order — the same bits everywhere.
// The passes over the tensors are the kernels above (bn_stats_kernel, bn_bwd_reduce_*, BnApply, BnBwdApply); only these folds are new.
// ------------------------------------------------------------------------- //
// row = the channel's `split` partials added in index order (bn_finalize_kernel's / bn_bwd_finalize_kernel's order), and the count
__global__ void bn_sync_fold_kernel(const double* __restrict__ partial, int C, int split, double count, double* __restrict__ row) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c == 0) row[2 * (int64_t)C] = count;
    if (c >= C) return;
    double s0 = 0, s1 = 0;
    for (int k = 0; k < split; ++k) { s0 += partial[((int64_t)c * split + k) * 2]; s1 += partial[((int64_t)c * split + k) * 2 + 1]; }
    row[c] = s0;
    row[C + c] = s1;
}

// row from the conv epilogue's per-tile fp32 sums stat[part][pitch][2], added in bn_partials_finalize_kernel's order (one block per channel)
__global__ __launch_bounds__(256) void bn_sync_partials_kernel(const float* __restrict__ stat, int nparts, int pitch, int C, double count, double* __restrict__ row) {
    __shared__ double red[8];
    const int c = blockIdx.x;
    double acc[2] = {0.0, 0.0};
    for (int p = threadIdx.x; p < nparts; p += 256) {
        const float2 v = *reinterpret_cast<const float2*>(stat + ((int64_t)p * pitch + c) * 2);
        acc[0] += (double)v.x;
        acc[1] += (double)v.y;
    }
    block_sum<2>(acc, red);
    if (threadIdx.x == 0) {
        if (c == 0) row[2 * (int64_t)C] = count;
        row[c] = acc[0];
        row[C + c] = acc[1];
    }
}

// rows[world][2C + 1] -> the statistics of the whole batch: sums and counts added in rank order, then bn_finalize_channel with the global count
__global__ void bn_sync_finalize_kernel(const double* __restrict__ rows, int world, int C, float eps, float momentum,
                                        float* __restrict__ save_mean, float* __restrict__ save_invstd,
                                        float* __restrict__ running_mean, float* __restrict__ running_var, int64_t* __restrict__ nbt) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c == 0 && nbt) *nbt += 1;
    if (c >= C) return;
    const int64_t len = 2 * (int64_t)C + 1;
    double s0 = 0, s1 = 0, count = 0;
    for (int r = 0; r < world; ++r) { s0 += rows[r * len + c]; s1 += rows[r * len + C + c]; count += rows[r * len + 2 * C]; }
    bn_finalize_channel(c, s0, s1, count, eps, momentum, save_mean, save_invstd, running_mean, running_var);
}

// backward: dbeta / dgamma = this rank's own sums (the gradient bucket adds the ranks later); coef[c] = {sum dz, sum dz * xhat} over ALL rows in
// rank order / the global count, for BnBwdApply
__global__ void bn_sync_bwd_coef_kernel(const double* __restrict__ rows, int world, int rank, int C,
                                        float* __restrict__ dgamma, float* __restrict__ dbeta, float* __restrict__ coef) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const int64_t len = 2 * (int64_t)C + 1;
    double s0 = 0, s1 = 0, count = 0;
    for (int r = 0; r < world; ++r) { s0 += rows[r * len + c]; s1 += rows[r * len + C + c]; count += rows[r * len + 2 * C]; }
    dbeta[c] = (float)rows[rank * len + c];
    dgamma[c] = (float)rows[rank * len + C + c];
    coef[2 * c] = (float)(s0 / count);
    coef[2 * c + 1] = (float)(s1 / count);
}

// ------------------------------------------------------------------------- //
// GAN loss: one block, value + gradient
// ------------------------------------------------------------------------- //
__global__ __launch_bounds__(256) void gan_loss_kernel(const float* __restrict__ y, int64_t n, int kind, float* __restrict__ loss_out, int accumulate, float* __restrict__ dy) {
    __shared__ double red[4];
    const float inv = 1.f / (float)n;
    double acc[1] = {0.0};
    for (int64_t i = threadIdx.x; i < n; i += 256) {
        const float v = y[i];
        float f, g;
        if (kind == 0 || kind == 4) {        // softplus(-v)
            f = fmaxf(-v, 0.f) + log1pf(expf(-fabsf(v)));
            g = -1.f / (1.f + expf(v));
        } else if (kind == 1) {              // softplus(v)
            f = fmaxf(v, 0.f) + log1pf(expf(-fabsf(v)));
            g = 1.f / (1.f + expf(-v));
        } else if (kind == 2) {              // relu(1 - v)
            f = fmaxf(1.f - v, 0.f);
            g = (1.f - v > 0.f) ? -1.f : 0.f;
        } else {                             // relu(1 + v)
            f = fmaxf(1.f + v, 0.f);
            g = (1.f + v > 0.f) ? 1.f : 0.f;
        }
        acc[0] += (double)f;
        if (dy) dy[i] = g * inv;
    }
    block_sum<1>(acc, red);
    if (threadIdx.x == 0) {
        const float val = (float)(acc[0] / (double)n);
        *loss_out = accumulate ? *loss_out + val : val;
    }
}

// ------------------------------------------------------------------------- //
// Adam
// ------------------------------------------------------------------------- //
// torch.optim.Adam's single-tensor update, operation for operation (torch/optim/adam.py _single_tensor_adam):
//   g' = g * gscale + wd * p ; m = lerp(m, g', 1 - b1) ; v = b2 * v + (1 - b2) * g' * g'
//   p -= step_size * m / (sqrt(v) / bc2_sqrt + eps)
// with the scalars (1 - b1, 1 - b2, step_size = lr / (1 - b1^t), bc2_sqrt) computed in double on the host and
// rounded once, as Python does.  fp contraction is off for this file's Adam code path (see adam_update).
struct AdamScalars {
    float w1, b2, w2, eps, wd, step_size, bc2_sqrt, gscale;   // w1 = 1 - beta1, w2 = 1 - beta2
};
__device__ __forceinline__ void adam_update(float& pi, float gi, float& mi, float& vi, const AdamScalars& k) {
#pragma clang fp contract(off)
    gi = gi * k.gscale;
    gi = gi + k.wd * pi;
    // at::lerp: weight < 0.5 ? a + w (b - a) : b - (b - a)(1 - w)
    const float d = gi - mi;
    mi = k.w1 < 0.5f ? mi + k.w1 * d : gi - d * (1.f - k.w1);
    vi = vi * k.b2;
    vi = vi + (k.w2 * gi) * gi;   // addcmul_(g, g, value): value * t1 * t2
    const float denom = sqrtf(vi) / k.bc2_sqrt + k.eps;
    pi = pi + (-k.step_size) * (mi / denom);
}
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, int64_t n,
                                                   const AdamScalars k) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        float pi = p[i], mi = m[i], vi = v[i];
        adam_update(pi, g[i], mi, vi, k);
        m[i] = mi; v[i] = vi; p[i] = pi;
    }
}

// up to ADAM_MT tensors of one optimiser in one launch (the DCVGAN models have ~100 small parameter tensors:
// one launch each was ~100 x 5 us of dispatch per step for 70 MB of state)
#define ADAM_MT 24
// THE multi-tensor table.  What every table shares, passed by value inside the kernel's own pack of pointers: the tensors' element counts and the
// prefix sum of their block counts.  A block is 256 threads; for the elementwise kernels it covers 4096 elements (MT_BLOCK), the spectral matrix-vector kernels
// count their own chunks in first_block.
#define MT_BLOCK 4096
struct MtTable {
    int64_t n[ADAM_MT];
    int32_t first_block[ADAM_MT + 1];
};
struct MtWhere {
    int t, blk;      // this block's tensor, and its index among that tensor's blocks
};
__device__ __forceinline__ MtWhere mt_where(const MtTable& k, int nt) {
    int t = 0;
    while (t + 1 < nt && (int)blockIdx.x >= k.first_block[t + 1]) ++t;
    return MtWhere{t, (int)blockIdx.x - k.first_block[t]};
}
// A block's (at most) 4096 elements from `base`, 16 per thread.  one(j) handles element j, quad(i) the four elements from i with 16-byte accesses.
// strided: element base + e * 256 + tid for e = 0 .. 15.
template <class One>
__device__ __forceinline__ void mt_strided(int64_t base, int64_t n, One one) {
#pragma unroll 4
    for (int e = 0; e < 16; ++e) {
        const int64_t i = base + e * 256 + threadIdx.x;
        if (i >= n) break;
        one(i);
    }
}
// `aligned` (the caller's predicate: every base the functors touch is on a 16-byte boundary, hence so is every block's first element): four quads per thread at
// base + (q * 256 + tid) * 4, the tensor's last 1..3 elements one at a time.  Otherwise one of exactly two orders.  MT_STRIDED hands a thread OTHER elements than
// the aligned branch does: right for kernels whose elements are independent (their results cannot depend on who computes them), and its accesses coalesce.
// MT_QUAD_ORDER visits the aligned branch's elements per thread in the aligned branch's order, one at a time: for a kernel that adds a thread's elements up in
// fp32, where the order is the result, so that the sum's bits do not depend on the alignment.  Do not swap one for the other: it changes bits.
// MT_STRIDED: ema_multi_kernel, sn_scale_kernel, sn_project_kernel (and, through mt_strided alone, the Adam kernels).  MT_QUAD_ORDER: guard_partial_kernel (a
// thread's fmaf chain of squares) and sn_inner_kernel.  tests/test_opt_exact_gpu.py holds the guard to it: the same gradients at an aligned and at a 4-byte-off base.
enum MtOrder { MT_STRIDED, MT_QUAD_ORDER };
template <MtOrder ORDER, class Quad, class One>
__device__ __forceinline__ void mt_traverse(int64_t base, int64_t n, bool aligned, Quad quad, One one) {
    if (aligned) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t i = base + (int64_t)(q * 256 + threadIdx.x) * 4;
            if (i + 4 <= n) {
                quad(i);
            } else {
                for (int64_t j = i; j < n; ++j) one(j);
            }
        }
    } else if (ORDER == MT_QUAD_ORDER) {
        for (int q = 0; q < 4; ++q) {
            const int64_t i = base + (int64_t)(q * 256 + threadIdx.x) * 4;
            for (int64_t j = i; j < i + 4 && j < n; ++j) one(j);
        }
    } else {
        mt_strided(base, n, one);
    }
}
__device__ __forceinline__ bool mt_aligned16(const void* a, const void* b = nullptr) {
    return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15) == 0;
}

// ---- the host side of the multi-tensor table (MtTable) ------------------------------------------------------------------------------------------------------
static int64_t mt_blocks(int64_t numel) { return (numel + MT_BLOCK - 1) / MT_BLOCK; }
// every table's block count fits the int the kernels index with (numels already known to be >= 0)
static bool mt_tables_fit(int n_tensors, const int64_t* numel) {
    int64_t blocks = 0;
    for (int t = 0; t < n_tensors; ++t) {
        blocks = (t % ADAM_MT ? blocks : 0) + mt_blocks(numel[t]);
        if (blocks > INT32_MAX) return false;
    }
    return true;
}
// Walks n_tensors in tables of ADAM_MT.  Per table: a zeroed Pack, fill(k, slot, tensor) sets the kernel's own fields of a slot (pointers, tab.n), first_block is
// the prefix sum of blocks_of(tensor); a table without blocks is skipped, every other goes to launch(k, nt, blocks, blocks of the tables before it), which returns
// what DCV_LAUNCH_CHECK gave.  Every check of the arguments belongs BEFORE the call: nothing here refuses.
template <class Pack, class Blocks, class Fill, class Launch>
static int mt_for_tables(int n_tensors, Blocks blocks_of, Fill fill, Launch launch) {
    int64_t before = 0;
    for (int t0 = 0; t0 < n_tensors; t0 += ADAM_MT) {
        Pack k;
        memset(&k, 0, sizeof(k));
        const int nt = std::min(ADAM_MT, n_tensors - t0);
        int blocks = 0;
        for (int t = 0; t < nt; ++t) {
            fill(k, t, t0 + t);
            k.tab.first_block[t] = blocks;
            blocks += (int)blocks_of(t0 + t);
        }
        k.tab.first_block[nt] = blocks;
        if (blocks == 0) continue;
        const int rc = launch(k, nt, blocks, before);
        if (rc != DCV_OK) return rc;
        before += blocks;
    }
    return DCV_OK;
}

struct AdamPack {
    float* p[ADAM_MT];
    const float* g[ADAM_MT];
    float* m[ADAM_MT];
    float* v[ADAM_MT];
    MtTable tab;
};
__device__ __forceinline__ void adam_multi_body(const AdamPack& k, int nt, const AdamScalars& sc) {
    const MtWhere at = mt_where(k.tab, nt);
    float* __restrict__ p = k.p[at.t];
    const float* __restrict__ g = k.g[at.t];
    float* __restrict__ m = k.m[at.t];
    float* __restrict__ v = k.v[at.t];
    mt_strided((int64_t)at.blk * MT_BLOCK, k.tab.n[at.t], [&](int64_t i) {      // (no 16-byte branch here)
        float pi = p[i], mi = m[i], vi = v[i];
        adam_update(pi, g[i], mi, vi, sc);
        m[i] = mi; v[i] = vi; p[i] = pi;
    });
}
__global__ __launch_bounds__(256) void adam_multi_kernel(const AdamPack k, int nt, const AdamScalars sc) { adam_multi_body(k, nt, sc); }

// ------------------------------------------------------------------------- //
// Gradient guard: global norm, clip coefficient, non-finite skip and loss-scale update, all decided on the device
// ------------------------------------------------------------------------- //
// Stage 1 (guard_partial_kernel): the multi-tensor table's block mapping (MtTable) over the gradients.  A thread
// squares and adds its (at most) 16 elements in fp32 and counts those whose exponent bits are all ones; the block combines both in double, in block_sum's fixed
// order, and stores ONE partial sum and ONE count.  Stage 2 (guard_decide_kernel): one workgroup adds the partials in a fixed order and writes the decision into
// the state array (DCV_GUARD_* in dcvgan_hip.h).  No atomics anywhere: the same gradients give the same bits.
struct GuardPack {
    const float* g[ADAM_MT];
    MtTable tab;
};
__device__ __forceinline__ void guard_take(float x, float& ss, int& bad) {
    // Explicitly fused, like ema_one.  Written `ss += x * x`, a thread's first two squares x0 x0 + x1 x1 may be contracted either way round (fma(x1, x1, x0 x0) or
    // fma(x0, x0, x1 x1)): the compiler's pick, and it moved with the code around this function.  This is the chain every build so far has computed.
    ss = fmaf(x, x, ss);
    bad += ((__float_as_uint(x) & 0x7f800000u) == 0x7f800000u) ? 1 : 0;
}
__global__ __launch_bounds__(256) void guard_partial_kernel(const GuardPack k, int nt, int block0, double* __restrict__ part, uint32_t* __restrict__ cnt) {
    __shared__ double red[8];
    const MtWhere at = mt_where(k.tab, nt);
    const float* __restrict__ g = k.g[at.t];
    float ss = 0.f;
    int bad = 0;
    mt_traverse<MT_QUAD_ORDER>((int64_t)at.blk * MT_BLOCK, k.tab.n[at.t], mt_aligned16(g),      // a sum: the bits must not depend on the alignment
        [&](int64_t i) {
            const float4 x = *reinterpret_cast<const float4*>(g + i);
            guard_take(x.x, ss, bad); guard_take(x.y, ss, bad); guard_take(x.z, ss, bad); guard_take(x.w, ss, bad);
        },
        [&](int64_t j) { guard_take(g[j], ss, bad); });
    double acc[2] = {(double)ss, (double)bad};      // (counts up to 4096: exact)
    block_sum<2>(acc, red);
    if (threadIdx.x == 0) {
        part[block0 + blockIdx.x] = acc[0];
        cnt[block0 + blockIdx.x] = (uint32_t)acc[1];
    }
}

struct GuardRule {
    double grad_scale, max_norm, growth, backoff;
    int32_t skip_nonfinite, dynamic, growth_interval;
};
__global__ __launch_bounds__(256) void guard_decide_kernel(const double* __restrict__ part, const uint32_t* __restrict__ cnt, int nb, const GuardRule r, float* __restrict__ state) {
    __shared__ double red[8];
    double acc[2] = {0.0, 0.0};
    for (int i = threadIdx.x; i < nb; i += 256) { acc[0] += part[i]; acc[1] += (double)cnt[i]; }
    block_sum<2>(acc, red);
    if (threadIdx.x != 0) return;
    const double ss = acc[0];
    const float scale = state[DCV_GUARD_LOSS_SCALE];      // the scale the measured backward ran with
    const double norm = sqrt(ss) * r.grad_scale / (double)scale;
    const bool bad = acc[1] > 0.0 || !isfinite(ss) || !isfinite((float)norm);
    double coef = 1.0;
    if (!bad && r.max_norm > 0.0) coef = fmin(1.0, r.max_norm / (norm + 1e-6));      // torch.nn.utils.clip_grad_norm_
    const bool skip = bad && r.skip_nonfinite;
    state[DCV_GUARD_GRAD_NORM] = (float)norm;
    state[DCV_GUARD_CLIP_COEF] = (float)coef;
    state[DCV_GUARD_FACTOR] = (float)(r.grad_scale * coef / (double)scale);
    state[DCV_GUARD_SKIPPED] = skip ? 1.f : 0.f;
    state[DCV_GUARD_SKIPPED_TOTAL] += skip ? 1.f : 0.f;
    state[DCV_GUARD_NONFINITE] = (float)acc[1];
    if (r.dynamic) {      // torch.amp.GradScaler's update (amp_update_scale): fp32 scale times double factor, rounded once; a growth that would overflow is not taken
        float tracker = state[DCV_GUARD_GROWTH_TRACKER], s = scale;
        if (bad) {
            s = (float)((double)s * r.backoff);
            tracker = 0.f;
        } else {
            tracker += 1.f;
            if (tracker >= (float)r.growth_interval) {
                const float grown = (float)((double)s * r.growth);
                if (isfinite(grown)) s = grown;
                tracker = 0.f;
            }
        }
        state[DCV_GUARD_LOSS_SCALE] = s;
        state[DCV_GUARD_GROWTH_TRACKER] = tracker;
    }
}

// The guarded Adam step.  guard_adam_prepare_kernel (one thread) reads the guard's decision; unless the step is skipped it advances the DEVICE step count and forms
// the AdamScalars from it in double — adam_scalars() below, on the device — with the guard's factor as gscale.  The update kernel reads them from the step block.
struct AdamStepBlock {      // 16 x 4 bytes, caller-owned (DCV_ADAM_STEP_BLOCK_BYTES); [0] is the step count a host may read back
    int32_t step, skip;
    AdamScalars sc;
    int32_t pad[6];
};
static_assert(sizeof(AdamStepBlock) == 64, "AdamStepBlock is the 64-byte block the header documents");
__global__ void guard_adam_prepare_kernel(AdamStepBlock* __restrict__ b, const float* __restrict__ state, double lr, double beta1, double beta2, double eps, double weight_decay) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int skip = state[DCV_GUARD_SKIPPED] != 0.f;
    b->skip = skip;
    if (skip) return;
    const int step = b->step + 1;
    b->step = step;
    const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
    AdamScalars k;
    k.w1 = (float)(1.0 - beta1);
    k.b2 = (float)beta2;
    k.w2 = (float)(1.0 - beta2);
    k.eps = (float)eps;
    k.wd = (float)weight_decay;
    k.step_size = (float)(lr / bc1);
    k.bc2_sqrt = (float)sqrt(bc2);
    k.gscale = state[DCV_GUARD_FACTOR];
    b->sc = k;
}
__global__ __launch_bounds__(256) void adam_multi_guarded_kernel(const AdamPack k, int nt, const AdamStepBlock* __restrict__ b) {
    if (b->skip) return;      // before any access to p, m or v
    const AdamScalars sc = b->sc;
    adam_multi_body(k, nt, sc);
}

// ------------------------------------------------------------------------- //
// EMA of model weights (the sampling twin): e += w (p - e), count, warm-up and skip decided on the device
// ------------------------------------------------------------------------- //
// ema_prepare_kernel (one thread, like guard_adam_prepare_kernel) reads the guard's decision; unless the update is skipped it takes the number of updates applied
// so far from the block, forms the weight 1 - d_t in double, rounds it once and advances the count.  ema_multi_kernel has the multi-tensor table's block mapping (MtTable); a
// tensor is either averaged (fp32) or copied dword for dword (BatchNorm running statistics, num_batches_tracked).  No atomics: the same inputs give the same bits.
struct EmaBlock {      // 16 x 4 bytes, caller-owned (DCV_EMA_BLOCK_BYTES); [0] is the number of updates applied, which a host may read back
    int32_t count, skip;
    float w;
    int32_t pad[13];
};
static_assert(sizeof(EmaBlock) == 64, "EmaBlock is the 64-byte block the header documents");
struct EmaPack {
    float* e[ADAM_MT];
    const float* s[ADAM_MT];
    MtTable tab;
    uint32_t copy_mask;      // bit t: tensor t is copied (mode 1), not averaged
};
__global__ void ema_prepare_kernel(EmaBlock* __restrict__ b, const float* __restrict__ state, double decay, int warmup) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int skip = state != nullptr && state[DCV_GUARD_SKIPPED] != 0.f;
    b->skip = skip;
    if (skip) return;
    const int t = b->count;
    const double d = warmup ? fmin(decay, (1.0 + (double)t) / (10.0 + (double)t)) : decay;
    b->w = (float)(1.0 - d);
    b->count = t + 1;
}
__device__ __forceinline__ float ema_one(float e, float p, float w) { return fmaf(w, p - e, e); }
__global__ __launch_bounds__(256) void ema_multi_kernel(const EmaPack k, int nt, const EmaBlock* __restrict__ b) {
    if (b->skip) return;      // before any access to a tensor
    const float w = b->w;
    const MtWhere at = mt_where(k.tab, nt);
    const int t = at.t;
    float* __restrict__ e = k.e[t];
    const float* __restrict__ s = k.s[t];
    const int64_t n = k.tab.n[t], base = (int64_t)at.blk * MT_BLOCK;
    const bool vec = mt_aligned16(e, s);
    if ((k.copy_mask >> t) & 1u) {      // bit patterns, no arithmetic
        uint32_t* __restrict__ eu = reinterpret_cast<uint32_t*>(e);
        const uint32_t* __restrict__ su = reinterpret_cast<const uint32_t*>(s);
        mt_traverse<MT_STRIDED>(base, n, vec,
            [&](int64_t i) { *reinterpret_cast<uint4*>(eu + i) = *reinterpret_cast<const uint4*>(su + i); },
            [&](int64_t j) { eu[j] = su[j]; });
        return;
    }
    mt_traverse<MT_STRIDED>(base, n, vec,
        [&](int64_t i) {
            const float4 p = *reinterpret_cast<const float4*>(s + i);
            float4 x = *reinterpret_cast<const float4*>(e + i);
            x.x = ema_one(x.x, p.x, w); x.y = ema_one(x.y, p.y, w); x.z = ema_one(x.z, p.z, w); x.w = ema_one(x.w, p.w, w);
            *reinterpret_cast<float4*>(e + i) = x;
        },
        [&](int64_t j) { e[j] = ema_one(e[j], s[j], w); });
}

// ------------------------------------------------------------------------- //
// Spectral normalisation of the discriminators' weights: power iteration, sigma, W_sn = W / sigma, and the gradient's projection
// ------------------------------------------------------------------------- //
// A weight is a matrix of M rows (cout) and K columns, contiguous.  Per table of up to ADAM_MT tensors:
//   sn_cols_kernel   t = W^T u      one block per SN_KC columns of a tensor; leaves t and the block's sum of t^2 (double) in the workspace
//   sn_rows_kernel   s = W v        one block per SN_MR rows (one wave each); v = t / max(|t|, eps); leaves s and the block's sum of s^2
//   sn_scale_kernel  u = s / max(|s|, eps); sigma = u^T s; W_sn = W / max(sigma, eps)     MtTable's block mapping over the M K elements
// Every block that needs a norm adds the tensor's block partials itself, all in the same fixed order (so all of them get the same bits), and one thread forms the
// square root and the reciprocal in double.  Products and a thread's running sums are fp32, everything above a thread is double.  No atomics.
// The first block of a tensor writes the vector (v, u, sigma) that its kernel has just normalised.
#define SN_KC 256      // columns per block of sn_cols_kernel (64 groups of 4 columns x 4 row phases)
#define SN_MR 4        // rows per block of sn_rows_kernel (one per wave)
struct SnPack {
    const float* w[ADAM_MT];
    float* w_sn[ADAM_MT];      // (project: const in effect)
    float* u[ADAM_MT];
    float* v[ADAM_MT];
    float* sigma[ADAM_MT];
    float* g[ADAM_MT];         // project only
    int32_t rows[ADAM_MT], cols[ADAM_MT];
    MtTable tab;               // n = rows * cols; first_block counts the launched kernel's own blocks (column chunks, row chunks or blocks of 4096 elements)
    int64_t ws_off[ADAM_MT];   // the tensor's part of the workspace, in doubles: [partials of t | partials of s or of <G, W_sn> | t (floats) | s (floats)]
};
__host__ __device__ __forceinline__ int sn_kchunks(int K) { return (K + SN_KC - 1) / SN_KC; }
__host__ __device__ __forceinline__ int sn_mchunks(int M) { return (M + SN_MR - 1) / SN_MR; }
__host__ __device__ __forceinline__ int64_t sn_eblocks(int M, int K) { return ((int64_t)M * K + MT_BLOCK - 1) / MT_BLOCK; }
// One tensor's workspace part, every array starting on a 16-byte boundary (counts in doubles, each rounded up to even; the part itself starts on an even offset of
// a 256-byte aligned buffer).  The second partial array serves the update's s (mchunks) and the projection's inner product (eblocks).
__host__ __device__ __forceinline__ int64_t sn_even(int64_t n) { return (n + 1) / 2 * 2; }
__host__ __device__ __forceinline__ int64_t sn_second(int M, int K) { return sn_even(sn_mchunks(M) > sn_eblocks(M, K) ? sn_mchunks(M) : sn_eblocks(M, K)); }
__host__ __device__ __forceinline__ int64_t sn_ws_doubles(int M, int K) {
    return sn_even(sn_kchunks(K)) + sn_second(M, K) + sn_even(((int64_t)K + 1) / 2) + sn_even(((int64_t)M + 1) / 2);
}
struct SnWs {
    double* part_t; double* part_s; float* t; float* s;
};
__device__ __forceinline__ SnWs sn_ws(double* ws, const SnPack& k, int ti) {
    const int M = k.rows[ti], K = k.cols[ti];
    SnWs r;
    r.part_t = ws + k.ws_off[ti];
    r.part_s = r.part_t + sn_even(sn_kchunks(K));
    double* t = r.part_s + sn_second(M, K);
    r.t = reinterpret_cast<float*>(t);
    r.s = reinterpret_cast<float*>(t + sn_even(((int64_t)K + 1) / 2));
    return r;
}
// sum of n doubles in a fixed order, the same in every block that asks; every thread gets it
__device__ __forceinline__ double sn_sum_partials(const double* __restrict__ p, int64_t n, double* red) {
    double acc[1] = {0.0};
    for (int64_t i = threadIdx.x; i < n; i += 256) acc[0] += p[i];
    block_sum<1>(acc, red);
    __syncthreads();      // red is reused by the caller
    return acc[0];
}
// 1 / max(sqrt(ss), eps), formed by one thread in double (correctly rounded sqrt, one division), rounded to fp32 once
__device__ __forceinline__ float sn_inv_norm(double ss, double eps, float* slot) {
    if (threadIdx.x == 0) *slot = (float)(1.0 / fmax(sqrt(ss), eps));
    __syncthreads();
    return *slot;
}

__global__ void sn_prepare_kernel(int32_t* __restrict__ skip, const float* __restrict__ state) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    *skip = state[DCV_GUARD_SKIPPED] != 0.f;
}

// t = W^T u.  from_s: u is s / max(|s|, eps) of the previous sn_rows_kernel (this kernel's first block of the tensor then stores it), else the stored u.
__global__ __launch_bounds__(256) void sn_cols_kernel(const SnPack k, int nt, int from_s, double eps, double* __restrict__ ws, const int32_t* __restrict__ skip) {
    if (skip != nullptr && *skip) return;
    __shared__ double red[8];
    __shared__ float inv_slot;
    __shared__ float part[4][SN_KC];
    const MtWhere at = mt_where(k.tab, nt);
    const int ti = at.t, chunk = at.blk;
    const int M = k.rows[ti], K = k.cols[ti];
    const float* __restrict__ w = k.w[ti];
    const SnWs a = sn_ws(ws, k, ti);
    float inv = 1.f;
    const float* __restrict__ usrc = k.u[ti];
    if (from_s) {
        inv = sn_inv_norm(sn_sum_partials(a.part_s, sn_mchunks(M), red), eps, &inv_slot);
        usrc = a.s;
        if (chunk == 0)
            for (int m = threadIdx.x; m < M; m += 256) k.u[ti][m] = a.s[m] * inv;
    }
    const int cg = threadIdx.x & 63, rp = threadIdx.x >> 6;
    const int col = chunk * SN_KC + cg * 4;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    if (((reinterpret_cast<uintptr_t>(w) & 15) == 0) && (K & 3) == 0) {      // base and row pitch on 16-byte boundaries: one 16-byte load per row
        if (col < K)
            for (int m = rp; m < M; m += 4) {
                const float um = usrc[m] * inv;
                const float4 x = *reinterpret_cast<const float4*>(w + (int64_t)m * K + col);
                acc[0] += x.x * um; acc[1] += x.y * um; acc[2] += x.z * um; acc[3] += x.w * um;
            }
    } else {
        for (int m = rp; m < M; m += 4) {
            const float um = usrc[m] * inv;
            const float* __restrict__ row = w + (int64_t)m * K;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (col + j < K) acc[j] += row[col + j] * um;
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) part[rp][cg * 4 + j] = acc[j];
    __syncthreads();
    const int c = chunk * SN_KC + threadIdx.x;
    float tv = 0.f;
    if (c < K) {
        tv = ((part[0][threadIdx.x] + part[1][threadIdx.x]) + part[2][threadIdx.x]) + part[3][threadIdx.x];
        a.t[c] = tv;
    }
    double ss[1] = {(double)tv * (double)tv};
    block_sum<1>(ss, red);
    if (threadIdx.x == 0) a.part_t[chunk] = ss[0];
}

// s = W v.  from_t: v is t / max(|t|, eps) of the previous sn_cols_kernel (this kernel's first block of the tensor then stores it), else the stored v.
__global__ __launch_bounds__(256) void sn_rows_kernel(const SnPack k, int nt, int from_t, double eps, double* __restrict__ ws, const int32_t* __restrict__ skip) {
    if (skip != nullptr && *skip) return;
    __shared__ double red[8];
    __shared__ float inv_slot;
    __shared__ float srow[SN_MR];
    const MtWhere at = mt_where(k.tab, nt);
    const int ti = at.t, chunk = at.blk;
    const int M = k.rows[ti], K = k.cols[ti];
    const float* __restrict__ w = k.w[ti];
    const SnWs a = sn_ws(ws, k, ti);
    float inv = 1.f;
    const float* __restrict__ vsrc = k.v[ti];
    if (from_t) {
        inv = sn_inv_norm(sn_sum_partials(a.part_t, sn_kchunks(K), red), eps, &inv_slot);
        vsrc = a.t;
        if (chunk == 0)
            for (int c = threadIdx.x; c < K; c += 256) k.v[ti][c] = a.t[c] * inv;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int m = chunk * SN_MR + wave;
    float acc = 0.f;
    if (m < M) {
        const float* __restrict__ row = w + (int64_t)m * K;
        if (((reinterpret_cast<uintptr_t>(w) & 15) == 0) && (K & 3) == 0 && ((reinterpret_cast<uintptr_t>(vsrc) & 15) == 0)) {
            for (int c = lane * 4; c < K; c += 256) {
                const float4 x = *reinterpret_cast<const float4*>(row + c);
                const float4 y = *reinterpret_cast<const float4*>(vsrc + c);
                acc += x.x * (y.x * inv); acc += x.y * (y.y * inv); acc += x.z * (y.z * inv); acc += x.w * (y.w * inv);
            }
        } else {      // the same elements per lane in the same order, one at a time: the bits do not depend on the alignment
            for (int c = lane * 4; c < K; c += 256)
                for (int j = 0; j < 4 && c + j < K; ++j) acc += row[c + j] * (vsrc[c + j] * inv);
        }
    }
    const double tot = wave_sum((double)acc);      // lanes' fp32 sums combined in double, fixed order
    if (lane == 0) {
        const float sv = (m < M) ? (float)tot : 0.f;
        srow[wave] = sv;
        if (m < M) a.s[m] = sv;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double ss = 0.0;
#pragma unroll
        for (int j = 0; j < SN_MR; ++j) ss += (double)srow[j] * (double)srow[j];
        a.part_s[chunk] = ss;
    }
}

// sigma = u^T s with u = s / max(|s|, eps) (from_s) or the stored u; W_sn = W * (float)(1 / max(sigma, eps))
__global__ __launch_bounds__(256) void sn_scale_kernel(const SnPack k, int nt, int from_s, double eps, double* __restrict__ ws, const int32_t* __restrict__ skip) {
    if (skip != nullptr && *skip) return;
    __shared__ double red[8];
    __shared__ float inv_slot, sig_slot;
    const MtWhere at = mt_where(k.tab, nt);
    const int ti = at.t, blk = at.blk;
    const int M = k.rows[ti];
    const SnWs a = sn_ws(ws, k, ti);
    float inv = 1.f;
    const float* __restrict__ usrc = k.u[ti];
    if (from_s) {
        inv = sn_inv_norm(sn_sum_partials(a.part_s, sn_mchunks(M), red), eps, &inv_slot);
        usrc = a.s;
    }
    double dot[1] = {0.0};
    for (int m = threadIdx.x; m < M; m += 256) dot[0] += (double)(usrc[m] * inv) * (double)a.s[m];
    block_sum<1>(dot, red);
    if (threadIdx.x == 0) {
        const float sg = (float)dot[0];
        sig_slot = sg;
        inv_slot = (float)(1.0 / fmax((double)sg, eps));
    }
    __syncthreads();
    const float isg = inv_slot;
    if (blk == 0) {
        if (from_s)
            for (int m = threadIdx.x; m < M; m += 256) k.u[ti][m] = a.s[m] * inv;
        if (threadIdx.x == 0) k.sigma[ti][0] = sig_slot;
    }
    const float* __restrict__ w = k.w[ti];
    float* __restrict__ o = k.w_sn[ti];
    mt_traverse<MT_STRIDED>((int64_t)blk * MT_BLOCK, k.tab.n[ti], mt_aligned16(w, o),
        [&](int64_t i) {
            float4 x = *reinterpret_cast<const float4*>(w + i);
            x.x *= isg; x.y *= isg; x.z *= isg; x.w *= isg;
            *reinterpret_cast<float4*>(o + i) = x;
        },
        [&](int64_t j) { o[j] = w[j] * isg; });
}

// The projection of a gradient G = dL/dW_sn onto the raw weight: dW = (G - <G, W_sn> u v^T) / max(sigma, eps), in place on G.
// sn_inner_kernel: per 4096-element block the partial <G, W_sn> (a thread's 16 products in fp32, double above); sn_project_kernel: every block adds its tensor's
// partials in the same order, one thread rounds the inner product and 1 / sigma to fp32, then g <- fmaf(-(c u_m), v_k, g) * (1 / sigma).
__global__ __launch_bounds__(256) void sn_inner_kernel(const SnPack k, int nt, double* __restrict__ ws) {
    __shared__ double red[8];
    const MtWhere at = mt_where(k.tab, nt);
    const int ti = at.t, blk = at.blk;
    const float* __restrict__ g = k.g[ti];
    const float* __restrict__ y = k.w_sn[ti];
    float acc = 0.f;
    mt_traverse<MT_QUAD_ORDER>((int64_t)blk * MT_BLOCK, k.tab.n[ti], mt_aligned16(g, y),      // a sum: the bits must not depend on the alignment
        [&](int64_t i) {
            const float4 a = *reinterpret_cast<const float4*>(g + i);
            const float4 b = *reinterpret_cast<const float4*>(y + i);
            acc += a.x * b.x; acc += a.y * b.y; acc += a.z * b.z; acc += a.w * b.w;
        },
        [&](int64_t j) { acc += g[j] * y[j]; });
    double s[1] = {(double)acc};
    block_sum<1>(s, red);
    if (threadIdx.x == 0) sn_ws(ws, k, ti).part_s[blk] = s[0];
}
__device__ __forceinline__ float sn_project_one(float g, float c, float um, float vk, float isg) { return fmaf(-(c * um), vk, g) * isg; }
__global__ __launch_bounds__(256) void sn_project_kernel(const SnPack k, int nt, double eps, double* __restrict__ ws) {
    __shared__ double red[8];
    __shared__ float c_slot, isg_slot;
    const MtWhere at = mt_where(k.tab, nt);
    const int ti = at.t, blk = at.blk;
    const int M = k.rows[ti], K = k.cols[ti];
    const double inner = sn_sum_partials(sn_ws(ws, k, ti).part_s, sn_eblocks(M, K), red);
    if (threadIdx.x == 0) {
        c_slot = (float)inner;
        isg_slot = (float)(1.0 / fmax((double)k.sigma[ti][0], eps));
    }
    __syncthreads();
    const float c = c_slot, isg = isg_slot;
    float* __restrict__ g = k.g[ti];
    const float* __restrict__ u = k.u[ti];
    const float* __restrict__ v = k.v[ti];
    mt_traverse<MT_STRIDED>((int64_t)blk * MT_BLOCK, k.tab.n[ti], mt_aligned16(g),
        [&](int64_t i) {
            float4 x = *reinterpret_cast<const float4*>(g + i);
            float e[4] = {x.x, x.y, x.z, x.w};
            int m = (int)(i / K), c0 = (int)(i - (int64_t)m * K);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                e[j] = sn_project_one(e[j], c, u[m], v[c0], isg);
                if (++c0 == K) { c0 = 0; ++m; }
            }
            x.x = e[0]; x.y = e[1]; x.z = e[2]; x.w = e[3];
            *reinterpret_cast<float4*>(g + i) = x;
        },
        [&](int64_t j) { const int m = (int)(j / K); g[j] = sn_project_one(g[j], c, u[m], v[(int)(j - (int64_t)m * K)], isg); });
}

// ------------------------------------------------------------------------- //
// GRU recurrence (dm <= 32): one 64-lane block per sample, lane u < dm owns unit u
// ------------------------------------------------------------------------- //
#define GRU_MAXD 32
__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }

__global__ __launch_bounds__(64) void gru_fwd_kernel(const float* __restrict__ e, const float* __restrict__ h0, const float* __restrict__ w_ih, const float* __restrict__ w_hh,
                                                     const float* __restrict__ b_ih, const float* __restrict__ b_hh, float* __restrict__ out, float* __restrict__ gates,
                                                     int T, int B, int dm) {
    __shared__ float h[GRU_MAXD], x[GRU_MAXD];
    const int b = blockIdx.x, u = threadIdx.x;
    if (u < dm) h[u] = h0[(int64_t)b * dm + u];
    __syncthreads();
    for (int t = 0; t < T; ++t) {
        if (u < dm) x[u] = e[((int64_t)t * B + b) * dm + u];
        __syncthreads();
        float hn_new = 0.f;
        if (u < dm) {
            float ir = b_ih[u], iz = b_ih[dm + u], in_ = b_ih[2 * dm + u];
            float hr = b_hh[u], hz = b_hh[dm + u], hn = b_hh[2 * dm + u];
            for (int k = 0; k < dm; ++k) {
                const float xk = x[k], hk = h[k];
                ir += w_ih[(int64_t)u * dm + k] * xk;
                iz += w_ih[(int64_t)(dm + u) * dm + k] * xk;
                in_ += w_ih[(int64_t)(2 * dm + u) * dm + k] * xk;
                hr += w_hh[(int64_t)u * dm + k] * hk;
                hz += w_hh[(int64_t)(dm + u) * dm + k] * hk;
                hn += w_hh[(int64_t)(2 * dm + u) * dm + k] * hk;
            }
            const float r = sigmoidf_(ir + hr), z = sigmoidf_(iz + hz);
            const float n = tanhf(in_ + r * hn);
            hn_new = n + z * (h[u] - n);
            float* gt = gates + ((int64_t)t * B + b) * 4 * dm;
            gt[u] = r; gt[dm + u] = z; gt[2 * dm + u] = n; gt[3 * dm + u] = hn;
            out[((int64_t)b * T + t) * dm + u] = hn_new;
        }
        __syncthreads();
        if (u < dm) h[u] = hn_new;
        __syncthreads();
    }
}

// per-sample BPTT; partial parameter gradients go to part[b][P], P = 6*dm*dm + 6*dm,
// layout [dw_ih (3dm*dm) | dw_hh (3dm*dm) | db_ih (3dm) | db_hh (3dm)]
__global__ __launch_bounds__(64) void gru_bwd_kernel(const float* __restrict__ dout, const float* __restrict__ e, const float* __restrict__ h0, const float* __restrict__ out,
                                                     const float* __restrict__ gates, const float* __restrict__ w_hh, float* __restrict__ part, int T, int B, int dm, int lds_acc) {
    __shared__ float dgh[3 * GRU_MAXD], dh[GRU_MAXD];
    extern __shared__ float gru_acc[];   // lds_acc: the sample's P partial sums (the same additions in the same order, just not through global memory)
    const int b = blockIdx.x, u = threadIdx.x;
    const int P = 6 * dm * dm + 6 * dm;
    float* pp = lds_acc ? gru_acc : part + (int64_t)b * P;
    for (int i = u; i < P; i += 64) pp[i] = 0.f;
    if (u < dm) dh[u] = 0.f;
    __syncthreads();
    for (int t = T - 1; t >= 0; --t) {
        float dr_pre = 0.f, dz_pre = 0.f, dn_pre = 0.f, dhn = 0.f, dh_keep = 0.f;
        if (u < dm) {
            const float* gt = gates + ((int64_t)t * B + b) * 4 * dm;
            const float r = gt[u], z = gt[dm + u], n = gt[2 * dm + u], hn = gt[3 * dm + u];
            const float hprev = t > 0 ? out[((int64_t)b * T + t - 1) * dm + u] : h0[(int64_t)b * dm + u];
            const float d = dout[((int64_t)b * T + t) * dm + u] + dh[u];
            const float dn = d * (1.f - z);
            const float dz = d * (hprev - n);
            dh_keep = d * z;
            dn_pre = dn * (1.f - n * n);
            dhn = dn_pre * r;
            dr_pre = dn_pre * hn * r * (1.f - r);
            dz_pre = dz * z * (1.f - z);
            dgh[u] = dr_pre; dgh[dm + u] = dz_pre; dgh[2 * dm + u] = dhn;
            // parameter gradients owned by this lane: rows u, dm+u, 2dm+u
            for (int k = 0; k < dm; ++k) {
                const float xk = e[((int64_t)t * B + b) * dm + k];
                const float hk = t > 0 ? out[((int64_t)b * T + t - 1) * dm + k] : h0[(int64_t)b * dm + k];
                pp[(int64_t)u * dm + k] += dr_pre * xk;
                pp[(int64_t)(dm + u) * dm + k] += dz_pre * xk;
                pp[(int64_t)(2 * dm + u) * dm + k] += dn_pre * xk;
                pp[3 * dm * dm + (int64_t)u * dm + k] += dr_pre * hk;
                pp[3 * dm * dm + (int64_t)(dm + u) * dm + k] += dz_pre * hk;
                pp[3 * dm * dm + (int64_t)(2 * dm + u) * dm + k] += dhn * hk;
            }
            float* pb = pp + 6 * dm * dm;
            pb[u] += dr_pre; pb[dm + u] += dz_pre; pb[2 * dm + u] += dn_pre;
            pb[3 * dm + u] += dr_pre; pb[4 * dm + u] += dz_pre; pb[5 * dm + u] += dhn;
        }
        __syncthreads();
        if (u < dm) {
            float s = dh_keep;
            for (int j = 0; j < 3 * dm; ++j) s += w_hh[(int64_t)j * dm + u] * dgh[j];
            dh[u] = s;
        }
        __syncthreads();
    }
    if (lds_acc) {
        float* out_p = part + (int64_t)b * P;
        for (int i = u; i < P; i += 64) out_p[i] = pp[i];
    }
}

__global__ void gru_reduce_kernel(const float* __restrict__ part, int B, int P, int dm, float* dw_ih, float* dw_hh, float* db_ih, float* db_hh) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    float s = 0.f;
    for (int b = 0; b < B; ++b) s += part[(int64_t)b * P + i];
    const int w = 3 * dm * dm;
    if (i < w) dw_ih[i] = s;
    else if (i < 2 * w) dw_hh[i - w] = s;
    else if (i < 2 * w + 3 * dm) db_ih[i - 2 * w] = s;
    else db_hh[i - 2 * w - 3 * dm] = s;
}


// ------------------------------------------------------------------------- //
// sampling path (util.py:58-79, 198-248): float videos -> uint8 on the device
// ------------------------------------------------------------------------- //
// out[b][c*rep + q][t][h][w] = uint8( (clip(x,-1,1) + 1) / 2 * 255 )   (numpy astype: truncation),
// the same fp32 operation order as the reference so the bytes are identical.  rep = 3 tiles a
// 1-channel depth video into RGB (util.py:219-222).
struct ToU8 {
    const float* x; uint8_t* out; RowView xv; int rep;
    template <int VEC> __device__ void apply(const RowMap& m, const Pos& p) const {
        float v[VEC];
        ld<VEC>(x + offs(m, xv, p), v);
        const int64_t plane = (int64_t)m.H * m.W;
        const int64_t col = m.inner == 1 ? (int64_t)p.h * m.W + p.w : p.col;
        for (int q = 0; q < rep; ++q) {
            uint8_t* o = out + ((((int64_t)p.n * m.C + p.c) * rep + q) * m.D + p.d) * plane + col;
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
                float t = fminf(fmaxf(v[i], -1.f), 1.f);
                t = __fmul_rn(__fmul_rn(__fadd_rn(t, 1.f), 0.5f), 255.f);
                o[i] = (uint8_t)(int)t;
            }
        }
    }
};

// per-frame min / max of the flow magnitude (one block per (b, t) frame)
__global__ __launch_bounds__(256) void flow_minmax_kernel(const float* __restrict__ f, RowView fv, int T, int HW, int W, float scale, float* __restrict__ mm) {
    __shared__ float smin[4], smax[4];
    const int b = blockIdx.x / T, t = blockIdx.x % T;
    float lo = 3.4e38f, hi = 0.f;
    for (int i = threadIdx.x; i < HW; i += 256) {
        const int64_t o = (int64_t)b * fv.sn + (int64_t)t * fv.sd + (int64_t)(i / W) * fv.sh + (int64_t)(i % W) * fv.sw;
        const float x = fminf(fmaxf(f[o], -1.f), 1.f) * scale, y = fminf(fmaxf(f[o + fv.sc], -1.f), 1.f) * scale;
        const float mg = sqrtf(x * x + y * y);
        lo = fminf(lo, mg); hi = fmaxf(hi, mg);
    }
    for (int o = 32; o > 0; o >>= 1) { lo = fminf(lo, __shfl_xor(lo, o, 64)); hi = fmaxf(hi, __shfl_xor(hi, o, 64)); }
    if ((threadIdx.x & 63) == 0) { smin[threadIdx.x >> 6] = lo; smax[threadIdx.x >> 6] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        mm[2 * blockIdx.x] = fminf(fminf(smin[0], smin[1]), fminf(smin[2], smin[3]));
        mm[2 * blockIdx.x + 1] = fmaxf(fmaxf(smax[0], smax[1]), fmaxf(smax[2], smax[3]));
    }
}

// util.visualize_optical_flow (util.py:143-170): hue = direction (OpenCV 8-bit H = degrees / 2),
// saturation 255, value = magnitude min-max normalised per frame; HSV -> RGB, uint8 (B,3,T,H,W).
__global__ __launch_bounds__(256) void flow_to_rgb_kernel(const float* __restrict__ f, RowView fv, int B, int T, int HW, int W, float scale,
                                                          const float* __restrict__ mm, uint8_t* __restrict__ out) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)B * T * HW) return;
    const int i = (int)(idx % HW);
    const int bt = (int)(idx / HW), b = bt / T, t = bt % T;
    const int64_t o = (int64_t)b * fv.sn + (int64_t)t * fv.sd + (int64_t)(i / W) * fv.sh + (int64_t)(i % W) * fv.sw;
    const float x = fminf(fmaxf(f[o], -1.f), 1.f) * scale, y = fminf(fmaxf(f[o + fv.sc], -1.f), 1.f) * scale;
    const float mg = sqrtf(x * x + y * y);
    float ang = atan2f(y, x);
    if (ang < 0.f) ang += 6.283185307179586f;
    const int Hh = (int)(ang * 180.f / 3.14159265358979f / 2.f) & 255;        // uint8 assignment truncates
    const float lo = mm[2 * bt], hi = mm[2 * bt + 1];
    const int V = hi > lo ? (int)((mg - lo) * (255.f / (hi - lo))) : 0;
    // HSV (H in [0,180), S = 255, V) -> RGB
    const float h6 = (float)Hh / 30.f;
    const int sec = ((int)h6) % 6;
    const float fr = h6 - floorf(h6), v = (float)V;
    const float p_ = 0.f, q_ = v * (1.f - fr), t_ = v * fr;
    float r, g, bl;
    switch (sec) {
        case 0: r = v; g = t_; bl = p_; break;
        case 1: r = q_; g = v; bl = p_; break;
        case 2: r = p_; g = v; bl = t_; break;
        case 3: r = p_; g = q_; bl = v; break;
        case 4: r = t_; g = p_; bl = v; break;
        default: r = v; g = p_; bl = q_; break;
    }
    const int64_t plane = (int64_t)T * HW;
    uint8_t* ob = out + ((int64_t)b * 3) * plane + (int64_t)t * HW + i;
    ob[0] = (uint8_t)(int)(r + 0.5f); ob[plane] = (uint8_t)(int)(g + 0.5f); ob[2 * plane] = (uint8_t)(int)(bl + 0.5f);
}


// ------------------------------------------------------------------------- //
// input pipeline (dataset.py:125-186): frames as read from disk -> training tensors
// ------------------------------------------------------------------------- //
// out[b][c][t][h][w] = float(in[b][t][h][w][c]) / div - sub   (numpy's fp32 operation order)
template <class TIN>
__global__ __launch_bounds__(256) void decode_video_kernel(const TIN* __restrict__ in, float* __restrict__ out, int64_t BT_per_B /*T*/, int64_t HW, int Cc, int64_t total, float div, float sub) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;   // index over (b, c, t, hw) of the output
    if (i >= total) return;
    const int64_t hw = i % HW;
    int64_t r = i / HW;
    const int64_t t = r % BT_per_B; r /= BT_per_B;
    const int c = (int)(r % Cc);
    const int64_t b = r / Cc;
    const float v = (float)in[((b * BT_per_B + t) * HW + hw) * Cc + c];
    out[i] = decode_value(v, div, sub);
}

// SURREAL depth (dataset.py:137-156): foreground = depth < 1e10; min-max of the foreground per clip
__global__ __launch_bounds__(256) void surreal_minmax_kernel(const float* __restrict__ d, int64_t per_clip, float* __restrict__ mm) {
    __shared__ float smin[4], smax[4];
    const float* p = d + (int64_t)blockIdx.x * per_clip;
    float lo = 3.4e38f, hi = -3.4e38f;
    for (int64_t i = threadIdx.x; i < per_clip; i += 256) {
        surreal_fold(p[i], lo, hi);
    }
    for (int o = 32; o > 0; o >>= 1) { lo = fminf(lo, __shfl_xor(lo, o, 64)); hi = fmaxf(hi, __shfl_xor(hi, o, 64)); }
    if ((threadIdx.x & 63) == 0) { smin[threadIdx.x >> 6] = lo; smax[threadIdx.x >> 6] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        mm[2 * blockIdx.x] = fminf(fminf(smin[0], smin[1]), fminf(smin[2], smin[3]));
        mm[2 * blockIdx.x + 1] = fmaxf(fmaxf(smax[0], smax[1]), fmaxf(smax[2], smax[3]));
    }
}
__global__ __launch_bounds__(256) void surreal_norm_kernel(const float* __restrict__ d, int64_t per_clip, int64_t total, const float* __restrict__ mm, float* __restrict__ out) {
#pragma clang fp contract(off)   // numpy rounds h*1.8 before subtracting; no fma
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int64_t b = i / per_clip;
    out[i] = surreal_value(d[i], mm[2 * b], mm[2 * b + 1]);
}


// ------------------------------------------------------------------------- //
// segmentation branch: reductions over the channel axis, one thread per position.
// Consecutive threads are consecutive w, so every per-channel access is coalesced.
// ------------------------------------------------------------------------- //
struct PosView {   // (n, c, d, h, w) view: element offset of channel 0 at a position, channel stride
    int64_t sn, sc, sd, sh, sw;
    int32_t C, D, H, W;
};
__device__ __forceinline__ int64_t pos_offset(const PosView& v, int64_t p) {
    const int w = (int)(p % v.W); p /= v.W;
    const int h = (int)(p % v.H); p /= v.H;
    const int d = (int)(p % v.D); p /= v.D;
    return p * v.sn + d * v.sd + h * v.sh + w * v.sw;
}
__device__ __forceinline__ int argmax_first(const float* __restrict__ x, int C, int64_t sc) {
    float best = x[0];
    int bi = 0;
    for (int c = 1; c < C; ++c) {
        const float v = x[c * sc];
        if (v > best) { best = v; bi = c; }   // strict: the first maximum wins, like torch.argmax / np.argmax
    }
    return bi;
}
// y = softmax(x) over channels (generator.py:75-76 nn.Softmax(dim=1))
__global__ __launch_bounds__(256) void softmax_c_fwd_kernel(const float* __restrict__ x, PosView xv, float* __restrict__ y, PosView yv, int64_t P) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    const float* xp = x + pos_offset(xv, p);
    float* yp = y + pos_offset(yv, p);
    float mx = xp[0];
    for (int c = 1; c < xv.C; ++c) mx = fmaxf(mx, xp[c * xv.sc]);
    float sum = 0.f;
    for (int c = 0; c < xv.C; ++c) {
        const float e = expf(xp[c * xv.sc] - mx);
        yp[c * yv.sc] = e;
        sum += e;
    }
    for (int c = 0; c < xv.C; ++c) yp[c * yv.sc] = yp[c * yv.sc] / sum;
}
// dx = y * (dy - sum_c dy * y)
__global__ __launch_bounds__(256) void softmax_c_bwd_kernel(const float* __restrict__ dy, PosView dv, const float* __restrict__ y, PosView yv,
                                                           float* __restrict__ dx, PosView xv, int64_t P) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    const float* dp = dy + pos_offset(dv, p);
    const float* yp = y + pos_offset(yv, p);
    float* xp = dx + pos_offset(xv, p);
    float dot = 0.f;
    for (int c = 0; c < dv.C; ++c) dot += dp[c * dv.sc] * yp[c * yv.sc];
    for (int c = 0; c < dv.C; ++c) xp[c * xv.sc] = yp[c * yv.sc] * (dp[c * dv.sc] - dot);
}
// one-hot (or softmax) maps -> {-1, +1} maps (generator.py:378-385)
__global__ __launch_bounds__(256) void segm_onehot_kernel(const float* __restrict__ x, PosView xv, float* __restrict__ y, PosView yv, int64_t P) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    const int bi = argmax_first(x + pos_offset(xv, p), xv.C, xv.sc);
    float* yp = y + pos_offset(yv, p);
    for (int c = 0; c < xv.C; ++c) yp[c * yv.sc] = c == bi ? 1.f : -1.f;
}
// argmax -> part colour (util.py:236-246); out uint8 (N, 3, D, H, W) contiguous; palette = C x 3 bytes
__global__ __launch_bounds__(256) void segm_color_kernel(const float* __restrict__ x, PosView xv, const uint8_t* __restrict__ palette,
                                                        uint8_t* __restrict__ out, int64_t P) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    const int bi = argmax_first(x + pos_offset(xv, p), xv.C, xv.sc);
    const int64_t plane = (int64_t)xv.D * xv.H * xv.W;
    const int64_t n = p / plane, r = p % plane;
    for (int k = 0; k < 3; ++k) out[(n * 3 + k) * plane + r] = palette[bi * 3 + k];
}
// dataset.py:176-181: label frames (T, H, W) uint8 -> one-hot float (C, T, H, W), per clip of a (B, T, H, W) batch
__global__ __launch_bounds__(256) void segm_decode_kernel(const uint8_t* __restrict__ labels, float* __restrict__ out, int C, int64_t per_clip, int64_t P) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    const int64_t b = p / per_clip, r = p % per_clip;
    const int l = labels[p];
    for (int c = 0; c < C; ++c) out[(b * C + c) * per_clip + r] = onehot_value(l, c);
}

}  // namespace dcv

using namespace dcv;

extern "C" {

size_t dcv_bn_workspace_bytes(int channels) {
    // partial sums: C * split * 2 doubles (split <= 2048) + coef (2C floats)
    return (size_t)(2048 + channels) * 2 * sizeof(double) * 2 + (size_t)channels * 2 * sizeof(float) + 512;
}

int dcv_act_forward(const float* x, const dcv_dims5* xd, float* y, const dcv_dims5* yd, int act, float slope, void* stream) {
    if (!x || !y || !xd || !yd || !same_shape(*xd, *yd)) return fail(DCV_EINVAL, "act_forward: bad arguments");
    const dcv_dims5* views[2] = {xd, yd};
    const void* ptrs[2] = {x, y};
    RowMap m = make_rowmap(*xd, views, 2, ptrs);
    ActFwd f{x, y, rv(*xd), rv(*yd), act, slope};
    return launch_ew(m, f, static_cast<hipStream_t>(stream));
}

int dcv_act_backward(const float* dy, const dcv_dims5* dyd, const float* y, const dcv_dims5* yd, float* dx, const dcv_dims5* dxd, int act, float slope, void* stream) {
    if (!dy || !y || !dx || !dyd || !yd || !dxd || !same_shape(*dyd, *yd) || !same_shape(*dyd, *dxd)) return fail(DCV_EINVAL, "act_backward: bad arguments");
    const dcv_dims5* views[3] = {dyd, yd, dxd};
    const void* ptrs[3] = {dy, y, dx};
    RowMap m = make_rowmap(*dyd, views, 3, ptrs);
    ActBwd f{dy, y, dx, rv(*dyd), rv(*yd), rv(*dxd), act, slope};
    return launch_ew(m, f, static_cast<hipStream_t>(stream));
}

int dcv_axpby(const float* x, const dcv_dims5* xd, float a, const float* z, const dcv_dims5* zd, float b, float* y, const dcv_dims5* yd, void* stream) {
    if (!x || !y || !xd || !yd || !same_shape(*xd, *yd) || (z && (!zd || !same_shape(*xd, *zd)))) return fail(DCV_EINVAL, "axpby: bad arguments");
    const dcv_dims5* views[3] = {xd, yd, z ? zd : xd};
    const void* ptrs[3] = {x, y, z ? z : x};
    RowMap m = make_rowmap(*xd, views, 3, ptrs);
    Axpby f{x, z, y, rv(*xd), z ? rv(*zd) : rv(*xd), rv(*yd), a, b};
    return launch_ew(m, f, static_cast<hipStream_t>(stream));
}

int dcv_noise_add(const float* x, const dcv_dims5* xd, float* y, const dcv_dims5* yd, float sigma, uint64_t seed, uint64_t offset, void* stream) {
    if (!x || !y || !xd || !yd || !same_shape(*xd, *yd)) return fail(DCV_EINVAL, "noise_add: bad arguments");
    const dcv_dims5* views[2] = {xd, yd};
    const void* ptrs[2] = {x, y};
    RowMap m = make_rowmap(*xd, views, 2, ptrs);
    NoiseAdd f{x, y, rv(*xd), rv(*yd), sigma, seed, offset};
    return launch_ew(m, f, static_cast<hipStream_t>(stream));
}

int dcv_normal_fill(float* out, int64_t n, uint64_t seed, uint64_t offset, void* stream) {
    if (!out || n < 0) return fail(DCV_EINVAL, "normal_fill: bad arguments");
    if (n == 0) return DCV_OK;
    const int64_t q = (n + 3) / 4;
    hipLaunchKernelGGL(normal_fill_kernel, dim3((unsigned)((q + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), out, n, seed, offset);
    DCV_LAUNCH_CHECK();
    return DCV_OK;
}

int dcv_normal_fill_many(float* out, int64_t n, int64_t count, uint64_t seed, uint64_t offset, void* stream) {
    if (!out || n < 0 || count < 0) return fail(DCV_EINVAL, "normal_fill_many: bad arguments");
    if (n == 0 || count == 0) return DCV_OK;
    const int64_t t = (n + 3) / 4 * count;
    if ((t + 255) / 256 >= (1ll << 31)) return fail(DCV_EUNSUPPORTED, "normal_fill_many: too many values for one launch");
    hipLaunchKernelGGL(normal_fill_many_kernel, dim3((unsigned)((t + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), out, n, count, seed, offset);
    DCV_LAUNCH_CHECK();
    return DCV_OK;
}

int dcv_dropout_mask(float* mask, int64_t n, float p, uint64_t seed, uint64_t offset, void* stream) {
    if (!mask || n < 0 || p < 0.f || p >= 1.f) return fail(DCV_EINVAL, "dropout_mask: bad arguments");
    if (n == 0) return DCV_OK;
    const int64_t q = (n + 3) / 4;
    hipLaunchKernelGGL(dropout_mask_kernel, dim3((unsigned)((q + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), mask, n, p, seed, offset);
    DCV_LAUNCH_CHECK();
    return DCV_OK;
}

int dcv_bn_act_forward(const float* x, const dcv_dims5* xd, float* y, const dcv_dims5* yd, const float* gamma, const float* beta,
                       float* running_mean, float* running_var, int64_t* num_batches_tracked, float* save_mean, float* save_invstd, const float* mask,
                       int training, float momentum, float eps, int act, float slope, void* ws, size_t ws_bytes, void* stream) {
    if (!x || !y || !gamma || !beta || !save_mean || !save_invstd || !same_shape(*xd, *yd)) return fail(DCV_EINVAL, "bn_act_forward: bad arguments");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int C = xd->c;
    const dcv_dims5* views[2] = {xd, yd};
    const void* ptrs[2] = {x, y};
    RowMap m = make_rowmap(*xd, views, 2, ptrs);
    if (m.groups >= (1ll << 32)) return fail(DCV_EUNSUPPORTED, "bn: tensor too large");
    if (training) {
        if (ws_bytes < dcv_bn_workspace_bytes(C) || !ws) return fail(DCV_EWORKSPACE, "bn_act_forward: workspace too small");
        ChanMap cm = make_chanmap(m);
        if (bn_small_ok(m, cm)) {
            const double cnt = (double)xd->n * xd->d * xd->h * xd->w;
            hipLaunchKernelGGL(bn_fwd_small_kernel, dim3(C), dim3(SMALL_NT), 0, s, cm, x, rv(*xd), y, rv(*yd), gamma, beta, running_mean, running_var, num_batches_tracked,
                               save_mean, save_invstd, mask, cnt, eps, momentum, act, slope);
            DCV_LAUNCH_CHECK();
            snprintf(g_last_kernel, sizeof(g_last_kernel), "bn_fwd_small_kernel (%lld groups per channel, one launch)", (long long)cm.per_chan);
            return DCV_OK;
        }
        double* partial = static_cast<double*>(ws);
        if (m.vec == 4) hipLaunchKernelGGL((bn_stats_kernel<4>), dim3(C * cm.split), dim3(256), 0, s, cm, x, rv(*xd), partial);
        else hipLaunchKernelGGL((bn_stats_kernel<1>), dim3(C * cm.split), dim3(256), 0, s, cm, x, rv(*xd), partial);
        DCV_LAUNCH_CHECK();
        const double count = (double)xd->n * xd->d * xd->h * xd->w;
        hipLaunchKernelGGL(bn_finalize_kernel, dim3((C + 255) / 256), dim3(256), 0, s, partial, C, cm.split, count, eps, momentum, save_mean, save_invstd, running_mean, running_var, num_batches_tracked);
        DCV_LAUNCH_CHECK();
        snprintf(g_last_kernel, sizeof(g_last_kernel), "bn_stats_kernel<%d> x %d blocks per channel + bn_finalize_kernel + BnApply %s", m.vec, cm.split, ew_name(m));
    } else {
        if (!running_mean || !running_var) return fail(DCV_EINVAL, "bn_act_forward: eval mode needs running stats");
        hipLaunchKernelGGL(bn_eval_stats_kernel, dim3((C + 255) / 256), dim3(256), 0, s, C, eps, running_mean, running_var, save_mean, save_invstd);
        DCV_LAUNCH_CHECK();
        snprintf(g_last_kernel, sizeof(g_last_kernel), "bn_eval_stats_kernel + BnApply %s", ew_name(m));
    }
    BnApply f{x, y, rv(*xd), rv(*yd), gamma, beta, save_mean, save_invstd, mask, act, slope};
    return launch_ew(m, f, s);
}

int dcv_bn_act_forward_stats(const float* x, const dcv_dims5* xd, float* y, const dcv_dims5* yd, const float* gamma, const float* beta,
                             float* running_mean, float* running_var, int64_t* num_batches_tracked, float* save_mean, float* save_invstd, const float* mask,
                             float momentum, float eps, int act, float slope, const float* stat, int nparts, int pitch,
                             void* ws, size_t ws_bytes, void* stream) {
    if (!x || !y || !gamma || !beta || !save_mean || !save_invstd || !stat || nparts < 1 || !same_shape(*xd, *yd) || pitch < xd->c)
        return fail(DCV_EINVAL, "bn_act_forward_stats: bad arguments");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int C = xd->c;
    const dcv_dims5* views[2] = {xd, yd};
    const void* ptrs[2] = {x, y};
    RowMap m = make_rowmap(*xd, views, 2, ptrs);
    if (m.groups >= (1ll << 32)) return fail(DCV_EUNSUPPORTED, "bn: tensor too large");
    (void)ws; (void)ws_bytes;
    const double count = (double)xd->n * xd->d * xd->h * xd->w;
    {
        const ChanMap cm = make_chanmap(m);
        if (bn_small_ok(m, cm)) {   // the channel fits one workgroup's registers: its own sums are as cheap as combining the conv's partials, and it is one launch
            hipLaunchKernelGGL(bn_fwd_small_kernel, dim3(C), dim3(SMALL_NT), 0, s, cm, x, rv(*xd), y, rv(*yd), gamma, beta, running_mean, running_var, num_batches_tracked,
                               save_mean, save_invstd, mask, count, eps, momentum, act, slope);
            DCV_LAUNCH_CHECK();
            snprintf(g_last_kernel, sizeof(g_last_kernel), "bn_fwd_small_kernel (%lld groups per channel, one launch; the %d partials are not read)", (long long)cm.per_chan, nparts);
            return DCV_OK;
        }
    }
    hipLaunchKernelGGL(bn_partials_finalize_kernel, dim3(C), dim3(256), 0, s, stat, nparts, pitch, count, eps, momentum, save_mean, save_invstd, running_mean, running_var,
                       num_batches_tracked);
    DCV_LAUNCH_CHECK();
    snprintf(g_last_kernel, sizeof(g_last_kernel), "bn_partials_finalize_kernel (%d partials, pitch %d) + BnApply %s", nparts, pitch, ew_name(m));
    BnApply f{x, y, rv(*xd), rv(*yd), gamma, beta, save_mean, save_invstd, mask, act, slope};
    return launch_ew(m, f, s);
}

// The two halves of dcv_bn_act_forward_stats as calls of their own, for a BatchNorm group whose OUTPUT is never written because its consumers normalise on load
// (dcv_conv_forward_bn / dcv_conv_backward_weight_bn / dcv_conv_backward_data_bn): statistics + running-statistics update only ...
int dcv_bn_forward_stats_only(const float* x, const dcv_dims5* xd, float* running_mean, float* running_var, int64_t* num_batches_tracked, float* save_mean, float* save_invstd,
                              float momentum, float eps, const float* stat, int nparts, int pitch, void* stream) {
    if (!x || !xd || !save_mean || !save_invstd || !stat || nparts < 1 || pitch < xd->c) return fail(DCV_EINVAL, "bn_forward_stats_only: bad arguments");
    const double count = (double)xd->n * xd->d * xd->h * xd->w;
    hipLaunchKernelGGL(bn_partials_finalize_kernel, dim3(xd->c), dim3(256), 0, static_cast<hipStream_t>(stream), stat, nparts, pitch, count, eps, momentum, save_mean, save_invstd,
                       running_mean, running_var, num_batches_tracked);
    DCV_LAUNCH_CHECK();
    snprintf(g_last_kernel, sizeof(g_last_kernel), "bn_partials_finalize_kernel (%d partials, pitch %d), statistics only", nparts, pitch);
    return DCV_OK;
}

// ... and the apply pass alone (y = act(mask * (x * sc + sh)) from saved statistics): the fallback that materialises such an output after all
int dcv_bn_apply(const float* x, const dcv_dims5* xd, float* y, const dcv_dims5* yd, const float* gamma, const float* beta, const float* save_mean, const float* save_invstd,
                 const float* mask, int act, float slope, void* stream) {
    if (!x || !y || !gamma || !beta || !save_mean || !save_invstd || !same_shape(*xd, *yd)) return fail(DCV_EINVAL, "bn_apply: bad arguments");
    const dcv_dims5* views[2] = {xd, yd};
    const void* ptrs[2] = {x, y};
    RowMap m = make_rowmap(*xd, views, 2, ptrs);
    if (m.groups >= (1ll << 32)) return fail(DCV_EUNSUPPORTED, "bn: tensor too large");
    snprintf(g_last_kernel, sizeof(g_last_kernel), "BnApply %s (saved statistics)", ew_name(m));
    BnApply f{x, y, rv(*xd), rv(*yd), gamma, beta, save_mean, save_invstd, mask, act, slope};
    return launch_ew(m, f, static_cast<hipStream_t>(stream));
}

int dcv_bn_act_backward(const float* dy, const dcv_dims5* dyd, const float* x, const dcv_dims5* xd, float* dx, const dcv_dims5* dxd,
                        const float* gamma, const float* beta, const float* save_mean, const float* save_invstd, const float* mask,
                        int training, int act, float slope, float* dgamma, float* dbeta, void* ws, size_t ws_bytes, void* stream) {
    if (!dy || !x || !dx || !gamma || !beta || !save_mean || !save_invstd || !dgamma || !dbeta || !same_shape(*dyd, *xd) || !same_shape(*dyd, *dxd))
        return fail(DCV_EINVAL, "bn_act_backward: bad arguments");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int C = xd->c;
    if (ws_bytes < dcv_bn_workspace_bytes(C) || !ws) return fail(DCV_EWORKSPACE, "bn_act_backward: workspace too small");
    const dcv_dims5* views[3] = {dyd, xd, dxd};
    const void* ptrs[3] = {dy, x, dx};
    RowMap m = make_rowmap(*xd, views, 3, ptrs);
    if (m.groups >= (1ll << 32)) return fail(DCV_EUNSUPPORTED, "bn: tensor too large");
    ChanMap cm = make_chanmap(m);
    if (bn_small_ok(m, cm)) {
        const double cnt = (double)xd->n * xd->d * xd->h * xd->w;
        hipLaunchKernelGGL(bn_bwd_small_kernel, dim3(C), dim3(SMALL_NT), 0, s, cm, dy, rv(*dyd), x, rv(*xd), dx, rv(*dxd), gamma, beta, save_mean, save_invstd, mask,
                           cnt, act, slope, training, dgamma, dbeta);
        DCV_LAUNCH_CHECK();
        snprintf(g_last_kernel, sizeof(g_last_kernel), "bn_bwd_small_kernel (%lld groups per channel, one launch)", (long long)cm.per_chan);
        return DCV_OK;
    }
    double* partial = static_cast<double*>(ws);
    float* coef = reinterpret_cast<float*>(static_cast<char*>(ws) + (size_t)(2048 + C) * 2 * sizeof(double) * 2);
    const bool rows_kernel = m.vec == 4 && m.inner != 1 && m.gpr % 256 == 0 && !ew_rows_off();
    if (rows_kernel)
        hipLaunchKernelGGL(bn_bwd_reduce_rows_kernel, dim3(C * cm.split), dim3(256), 0, s, cm, dy, rv(*dyd), x, rv(*xd), gamma, beta, save_mean, save_invstd, mask, act, slope, partial);
    else if (m.vec == 4)
        hipLaunchKernelGGL((bn_bwd_reduce_kernel<4>), dim3(C * cm.split), dim3(256), 0, s, cm, dy, rv(*dyd), x, rv(*xd), gamma, beta, save_mean, save_invstd, mask, act, slope, partial);
    else
        hipLaunchKernelGGL((bn_bwd_reduce_kernel<1>), dim3(C * cm.split), dim3(256), 0, s, cm, dy, rv(*dyd), x, rv(*xd), gamma, beta, save_mean, save_invstd, mask, act, slope, partial);
    DCV_LAUNCH_CHECK();
    const double count = (double)xd->n * xd->d * xd->h * xd->w;
    hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3((C + 255) / 256), dim3(256), 0, s, partial, C, cm.split, count, dgamma, dbeta, coef);
    DCV_LAUNCH_CHECK();
    if (rows_kernel) snprintf(g_last_kernel, sizeof(g_last_kernel), "bn_bwd_reduce_rows_kernel x %d blocks per channel + bn_bwd_finalize_kernel + BnBwdApply %s", cm.split, ew_name(m));
    else snprintf(g_last_kernel, sizeof(g_last_kernel), "bn_bwd_reduce_kernel<%d> x %d blocks per channel + bn_bwd_finalize_kernel + BnBwdApply %s", m.vec, cm.split, ew_name(m));
    BnBwdApply f{dy, x, dx, rv(*dyd), rv(*xd), rv(*dxd), gamma, beta, save_mean, save_invstd, mask, coef, act, slope, training};
    return launch_ew(m, f, s);
}

// ---- synchronised BatchNorm: see the kernels' comment.  Every argument and workspace check comes before the first launch. ----
size_t dcv_bn_sync_row_doubles(int channels) { return channels > 0 ? 2 * (size_t)channels + 1 : 0; }

int dcv_bn_sync_sums(const float* x, const dcv_dims5* xd, const float* stat, int nparts, int pitch, double* row, void* ws, size_t ws_bytes, void* stream) {
    if (!x || !xd || !row || xd->c < 1 || numel(*xd) < 1 || (stat && (nparts < 1 || pitch < xd->c))) return fail(DCV_EINVAL, "bn_sync_sums: bad arguments");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int C = xd->c;
    const double count = (double)xd->n * xd->d * xd->h * xd->w;
    if (stat) {
        hipLaunchKernelGGL(bn_sync_partials_kernel, dim3(C), dim3(256), 0, s, stat, nparts, pitch, C, count, row);
        DCV_LAUNCH_CHECK();
        snprintf(g_last_kernel, sizeof(g_last_kernel), "bn_sync_partials_kernel (%d conv-epilogue partials per channel -> rank row)", nparts);
        return DCV_OK;
    }
    if (ws_bytes < dcv_bn_workspace_bytes(C) || !ws) return fail(DCV_EWORKSPACE, "bn_sync_sums: workspace too small");
    const dcv_dims5* views[1] = {xd};
    const void* ptrs[1] = {x};
    RowMap m = make_rowmap(*xd, views, 1, ptrs);
    if (m.groups >= (1ll << 32)) return fail(DCV_EUNSUPPORTED, "bn: tensor too large");
    ChanMap cm = make_chanmap(m);
    double* partial = static_cast<double*>(ws);
    if (m.vec == 4) hipLaunchKernelGGL((bn_stats_kernel<4>), dim3(C * cm.split), dim3(256), 0, s, cm, x, rv(*xd), partial);
    else hipLaunchKernelGGL((bn_stats_kernel<1>), dim3(C * cm.split), dim3(256), 0, s, cm, x, rv(*xd), partial);
    DCV_LAUNCH_CHECK();
    hipLaunchKernelGGL(bn_sync_fold_kernel, dim3((C + 255) / 256), dim3(256), 0, s, partial, C, cm.split, count, row);
    DCV_LAUNCH_CHECK();
    snprintf(g_last_kernel, sizeof(g_last_kernel), "bn_stats_kernel<%d> x %d blocks per channel + bn_sync_fold_kernel (rank row)", m.vec, cm.split);
    return DCV_OK;
}

int dcv_bn_sync_finalize(const double* rows, int world, int channels, float eps, float momentum, float* running_mean, float* running_var, int64_t* num_batches_tracked,
                         float* save_mean, float* save_invstd, void* stream) {
    if (!rows || world < 1 || channels < 1 || !save_mean || !save_invstd || (!running_mean) != (!running_var)) return fail(DCV_EINVAL, "bn_sync_finalize: bad arguments");
    hipLaunchKernelGGL(bn_sync_finalize_kernel, dim3((channels + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), rows, world, channels, eps, momentum,
                       save_mean, save_invstd, running_mean, running_var, num_batches_tracked);
    DCV_LAUNCH_CHECK();
    snprintf(g_last_kernel, sizeof(g_last_kernel), "bn_sync_finalize_kernel (%d rank rows in rank order)", world);
    return DCV_OK;
}

int dcv_bn_sync_backward_sums(const float* dy, const dcv_dims5* dyd, const float* x, const dcv_dims5* xd, const float* gamma, const float* beta,
                              const float* save_mean, const float* save_invstd, const float* mask, int act, float slope, double* row,
                              void* ws, size_t ws_bytes, void* stream) {
    if (!dy || !dyd || !x || !xd || !gamma || !beta || !save_mean || !save_invstd || !row || !same_shape(*dyd, *xd) || numel(*xd) < 1)
        return fail(DCV_EINVAL, "bn_sync_backward_sums: bad arguments");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int C = xd->c;
    if (ws_bytes < dcv_bn_workspace_bytes(C) || !ws) return fail(DCV_EWORKSPACE, "bn_sync_backward_sums: workspace too small");
    const dcv_dims5* views[2] = {dyd, xd};
    const void* ptrs[2] = {dy, x};
    RowMap m = make_rowmap(*xd, views, 2, ptrs);
    if (m.groups >= (1ll << 32)) return fail(DCV_EUNSUPPORTED, "bn: tensor too large");
    ChanMap cm = make_chanmap(m);
    double* partial = static_cast<double*>(ws);
    const bool rows_kernel = m.vec == 4 && m.inner != 1 && m.gpr % 256 == 0 && !ew_rows_off();
    if (rows_kernel)
        hipLaunchKernelGGL(bn_bwd_reduce_rows_kernel, dim3(C * cm.split), dim3(256), 0, s, cm, dy, rv(*dyd), x, rv(*xd), gamma, beta, save_mean, save_invstd, mask, act, slope, partial);
    else if (m.vec == 4)
        hipLaunchKernelGGL((bn_bwd_reduce_kernel<4>), dim3(C * cm.split), dim3(256), 0, s, cm, dy, rv(*dyd), x, rv(*xd), gamma, beta, save_mean, save_invstd, mask, act, slope, partial);
    else
        hipLaunchKernelGGL((bn_bwd_reduce_kernel<1>), dim3(C * cm.split), dim3(256), 0, s, cm, dy, rv(*dyd), x, rv(*xd), gamma, beta, save_mean, save_invstd, mask, act, slope, partial);
    DCV_LAUNCH_CHECK();
    const double count = (double)xd->n * xd->d * xd->h * xd->w;
    hipLaunchKernelGGL(bn_sync_fold_kernel, dim3((C + 255) / 256), dim3(256), 0, s, partial, C, cm.split, count, row);
    DCV_LAUNCH_CHECK();
    if (rows_kernel) snprintf(g_last_kernel, sizeof(g_last_kernel), "bn_bwd_reduce_rows_kernel x %d blocks per channel + bn_sync_fold_kernel (rank row)", cm.split);
    else snprintf(g_last_kernel, sizeof(g_last_kernel), "bn_bwd_reduce_kernel<%d> x %d blocks per channel + bn_sync_fold_kernel (rank row)", m.vec, cm.split);
    return DCV_OK;
}

int dcv_bn_sync_backward_apply(const float* dy, const dcv_dims5* dyd, const float* x, const dcv_dims5* xd, float* dx, const dcv_dims5* dxd,
                               const float* gamma, const float* beta, const float* save_mean, const float* save_invstd, const float* mask, int act, float slope,
                               const double* rows, int world, int rank, float* dgamma, float* dbeta, void* ws, size_t ws_bytes, void* stream) {
    if (!dy || !dyd || !x || !xd || !dx || !dxd || !gamma || !beta || !save_mean || !save_invstd || !rows || world < 1 || rank < 0 || rank >= world || !dgamma || !dbeta
        || !same_shape(*dyd, *xd) || !same_shape(*dyd, *dxd) || numel(*xd) < 1)
        return fail(DCV_EINVAL, "bn_sync_backward_apply: bad arguments");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int C = xd->c;
    if (ws_bytes < dcv_bn_workspace_bytes(C) || !ws) return fail(DCV_EWORKSPACE, "bn_sync_backward_apply: workspace too small");
    const dcv_dims5* views[3] = {dyd, xd, dxd};
    const void* ptrs[3] = {dy, x, dx};
    RowMap m = make_rowmap(*xd, views, 3, ptrs);
    if (m.groups >= (1ll << 32)) return fail(DCV_EUNSUPPORTED, "bn: tensor too large");
    float* coef = reinterpret_cast<float*>(static_cast<char*>(ws) + (size_t)(2048 + C) * 2 * sizeof(double) * 2);      // where dcv_bn_act_backward keeps it
    hipLaunchKernelGGL(bn_sync_bwd_coef_kernel, dim3((C + 255) / 256), dim3(256), 0, s, rows, world, rank, C, dgamma, dbeta, coef);
    DCV_LAUNCH_CHECK();
    snprintf(g_last_kernel, sizeof(g_last_kernel), "bn_sync_bwd_coef_kernel (%d rank rows, own row %d) + BnBwdApply", world, rank);
    BnBwdApply f{dy, x, dx, rv(*dyd), rv(*xd), rv(*dxd), gamma, beta, save_mean, save_invstd, mask, coef, act, slope, 1};
    return launch_ew(m, f, s);
}

// y[i] = x[i] * *s: the chain rule through a loss term — the upstream cotangent is a 0-d DEVICE tensor (loss.backward(), trainer.py:319,356)
__global__ __launch_bounds__(256) void scale_dev_kernel(const float* __restrict__ x, int64_t n, const float* __restrict__ s, float* __restrict__ y) {
    const float k = *s;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) y[i] = x[i] * k;
}

int dcv_scale_dev(const float* x, int64_t n, const float* s, float* y, void* stream) {
    if (!x || !s || !y || n < 0) return fail(DCV_EINVAL, "scale_dev: bad arguments");
    if (n == 0) return DCV_OK;
    hipLaunchKernelGGL(scale_dev_kernel, dim3(grid_for(n)), dim3(256), 0, static_cast<hipStream_t>(stream), x, n, s, y);
    DCV_LAUNCH_CHECK();
    return DCV_OK;
}

int dcv_gan_loss(const float* y, int64_t n, int kind, float* loss_out, int accumulate, float* dy_out, void* stream) {
    if (!y || !loss_out || n < 1 || kind < 0 || kind > 4) return fail(DCV_EINVAL, "gan_loss: bad arguments");
    hipLaunchKernelGGL(gan_loss_kernel, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream), y, n, kind, loss_out, accumulate, dy_out);
    DCV_LAUNCH_CHECK();
    return DCV_OK;
}

// bias corrections and step size in double, rounded once (torch computes them as Python floats)
static AdamScalars adam_scalars(double lr, double beta1, double beta2, double eps, double weight_decay, int step, double grad_scale) {
    AdamScalars k;
    const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
    k.w1 = (float)(1.0 - beta1);
    k.b2 = (float)beta2;
    k.w2 = (float)(1.0 - beta2);
    k.eps = (float)eps;
    k.wd = (float)weight_decay;
    k.step_size = (float)(lr / bc1);
    k.bc2_sqrt = (float)sqrt(bc2);
    k.gscale = (float)grad_scale;
    return k;
}

int dcv_adam_step(float* p, const float* g, float* m, float* v, int64_t n, double lr, double beta1, double beta2, double eps, double weight_decay,
                  int step, double grad_scale, void* stream) {
    if (!p || !g || !m || !v || n < 0 || step < 1) return fail(DCV_EINVAL, "adam_step: bad arguments");
    if (n == 0) return DCV_OK;
    const AdamScalars k = adam_scalars(lr, beta1, beta2, eps, weight_decay, step, grad_scale);
    hipLaunchKernelGGL(adam_kernel, dim3(grid_for(n)), dim3(256), 0, static_cast<hipStream_t>(stream), p, g, m, v, n, k);
    DCV_LAUNCH_CHECK();
    return DCV_OK;
}


// both Adam entry points: every tensor checked before the first launch
static int adam_tensors_ok(const char* who, int n_tensors, float* const* p, const float* const* g, float* const* m, float* const* v, const int64_t* numel) {
    for (int t = 0; t < n_tensors; ++t)
        if (!p[t] || !g[t] || !m[t] || !v[t] || numel[t] < 0) return fail(DCV_EINVAL, "%s: null tensor", who);
    if (!mt_tables_fit(n_tensors, numel)) return fail(DCV_EINVAL, "%s: too many elements", who);
    return DCV_OK;
}
static auto adam_fill(float* const* p, const float* const* g, float* const* m, float* const* v, const int64_t* numel) {
    return [=](AdamPack& k, int t, int i) { k.p[t] = p[i]; k.g[t] = g[i]; k.m[t] = m[i]; k.v[t] = v[i]; k.tab.n[t] = numel[i]; };
}

int dcv_adam_step_multi(int n_tensors, float* const* p, const float* const* g, float* const* m, float* const* v, const int64_t* numel,
                        double lr, double beta1, double beta2, double eps, double weight_decay, int step, double grad_scale, void* stream) {
    if (n_tensors < 0 || (n_tensors > 0 && (!p || !g || !m || !v || !numel)) || step < 1) return fail(DCV_EINVAL, "adam_step_multi: bad arguments");
    if (const int rc = adam_tensors_ok("adam_step_multi", n_tensors, p, g, m, v, numel)) return rc;
    const AdamScalars sc = adam_scalars(lr, beta1, beta2, eps, weight_decay, step, grad_scale);
    return mt_for_tables<AdamPack>(n_tensors, [&](int i) { return mt_blocks(numel[i]); }, adam_fill(p, g, m, v, numel),
        [&](const AdamPack& k, int nt, int blocks, int64_t) {
            hipLaunchKernelGGL(adam_multi_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), k, nt, sc);
            DCV_LAUNCH_CHECK();
            return DCV_OK;
        });
}

// blocks of stage 1 <= total / 4096 + one ragged block per tensor; a double and a count for each
static int64_t guard_max_blocks(int64_t total_elements, int n_tensors) { return total_elements / 4096 + n_tensors; }

size_t dcv_grad_guard_workspace_bytes(int64_t total_elements, int n_tensors) {
    if (total_elements < 0 || n_tensors < 0) { fail(DCV_EINVAL, "grad_guard_workspace_bytes: bad arguments"); return 0; }
    return align_up((size_t)std::max<int64_t>(1, guard_max_blocks(total_elements, n_tensors)) * (sizeof(double) + sizeof(uint32_t)), 256);
}

int dcv_grad_guard_measure(int n_tensors, const float* const* g, const int64_t* numel, double grad_scale, double max_norm, int skip_nonfinite, int dynamic,
                           double growth_factor, double backoff_factor, int growth_interval, float* state, void* ws, size_t ws_bytes, void* stream) {
    if (n_tensors < 0 || (n_tensors > 0 && (!g || !numel)) || !state || !ws || !(grad_scale > 0.0) || (dynamic && (!(growth_factor > 0.0) || !(backoff_factor > 0.0) || growth_interval < 1)))
        return fail(DCV_EINVAL, "grad_guard_measure: bad arguments");
    int64_t nb = 0;
    for (int t = 0; t < n_tensors; ++t) {
        if (!g[t] || numel[t] < 0) return fail(DCV_EINVAL, "grad_guard_measure: null tensor");
        nb += mt_blocks(numel[t]);
    }
    if (nb > INT32_MAX) return fail(DCV_EINVAL, "grad_guard_measure: too many elements");
    if ((size_t)nb * (sizeof(double) + sizeof(uint32_t)) > ws_bytes) return fail(DCV_EWORKSPACE, "grad_guard_measure: workspace too small");
    hipStream_t s = static_cast<hipStream_t>(stream);
    double* part = static_cast<double*>(ws);
    uint32_t* cnt = reinterpret_cast<uint32_t*>(part + nb);
    const int rc = mt_for_tables<GuardPack>(n_tensors, [&](int i) { return mt_blocks(numel[i]); },
        [&](GuardPack& k, int t, int i) { k.g[t] = g[i]; k.tab.n[t] = numel[i]; },
        [&](const GuardPack& k, int nt, int blocks, int64_t block0) {
            hipLaunchKernelGGL(guard_partial_kernel, dim3((unsigned)blocks), dim3(256), 0, s, k, nt, (int)block0, part, cnt);
            DCV_LAUNCH_CHECK();
            return DCV_OK;
        });
    if (rc != DCV_OK) return rc;
    const GuardRule r{grad_scale, max_norm, growth_factor, backoff_factor, skip_nonfinite ? 1 : 0, dynamic ? 1 : 0, growth_interval};
    hipLaunchKernelGGL(guard_decide_kernel, dim3(1), dim3(256), 0, s, part, cnt, (int)nb, r, state);
    DCV_LAUNCH_CHECK();
    return DCV_OK;
}

int dcv_adam_step_multi_guarded(int n_tensors, float* const* p, const float* const* g, float* const* m, float* const* v, const int64_t* numel,
                                double lr, double beta1, double beta2, double eps, double weight_decay, int32_t* step_block, const float* state, void* stream) {
    if (n_tensors < 0 || (n_tensors > 0 && (!p || !g || !m || !v || !numel)) || !step_block || !state) return fail(DCV_EINVAL, "adam_step_multi_guarded: bad arguments");
    if (const int rc = adam_tensors_ok("adam_step_multi_guarded", n_tensors, p, g, m, v, numel)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    AdamStepBlock* b = reinterpret_cast<AdamStepBlock*>(step_block);
    hipLaunchKernelGGL(guard_adam_prepare_kernel, dim3(1), dim3(1), 0, s, b, state, lr, beta1, beta2, eps, weight_decay);
    DCV_LAUNCH_CHECK();
    return mt_for_tables<AdamPack>(n_tensors, [&](int i) { return mt_blocks(numel[i]); }, adam_fill(p, g, m, v, numel),
        [&](const AdamPack& k, int nt, int blocks, int64_t) {
            hipLaunchKernelGGL(adam_multi_guarded_kernel, dim3((unsigned)blocks), dim3(256), 0, s, k, nt, b);
            DCV_LAUNCH_CHECK();
            return DCV_OK;
        });
}

int dcv_ema_update_multi(int n_tensors, float* const* ema, const float* const* src, const int64_t* numel, const int32_t* mode,
                         double decay, int warmup, int32_t* ema_block, const float* guard_state, void* stream) {
    if (n_tensors < 0 || (n_tensors > 0 && (!ema || !src || !numel || !mode)) || !(decay >= 0.0 && decay < 1.0) || !ema_block)
        return fail(DCV_EINVAL, "ema_update_multi: bad arguments");
    for (int t = 0; t < n_tensors; ++t) {      // every check before any launch
        if (numel[t] < 0 || (numel[t] > 0 && (!ema[t] || !src[t]))) return fail(DCV_EINVAL, "ema_update_multi: null tensor or negative numel");
        if (mode[t] != 0 && mode[t] != 1) return fail(DCV_EINVAL, "ema_update_multi: mode must be 0 (average) or 1 (copy)");
    }
    if (!mt_tables_fit(n_tensors, numel)) return fail(DCV_EINVAL, "ema_update_multi: too many elements");
    hipStream_t s = static_cast<hipStream_t>(stream);
    EmaBlock* b = reinterpret_cast<EmaBlock*>(ema_block);
    hipLaunchKernelGGL(ema_prepare_kernel, dim3(1), dim3(1), 0, s, b, guard_state, decay, warmup ? 1 : 0);
    DCV_LAUNCH_CHECK();
    return mt_for_tables<EmaPack>(n_tensors, [&](int i) { return mt_blocks(numel[i]); },
        [&](EmaPack& k, int t, int i) {
            k.e[t] = ema[i]; k.s[t] = src[i]; k.tab.n[t] = numel[i];
            if (mode[i]) k.copy_mask |= 1u << t;
        },
        [&](const EmaPack& k, int nt, int blocks, int64_t) {
            hipLaunchKernelGGL(ema_multi_kernel, dim3((unsigned)blocks), dim3(256), 0, s, k, nt, b);
            DCV_LAUNCH_CHECK();
            return DCV_OK;
        });
}

// workspace: 256 bytes (the skip flag), then every tensor's part (sn_ws_doubles)
static bool sn_shapes_ok(int n, const int32_t* rows, const int32_t* cols) {
    if (n < 0 || (n > 0 && (!rows || !cols))) return false;
    for (int t = 0; t < n; ++t)
        if (rows[t] < 1 || cols[t] < 1 || (int64_t)rows[t] * cols[t] > (int64_t)1 << 30) return false;
    return true;
}
static size_t sn_workspace_bytes(int n, const int32_t* rows, const int32_t* cols) {
    int64_t d = 0;
    for (int t = 0; t < n; ++t) d += sn_ws_doubles(rows[t], cols[t]);
    return align_up(256 + (size_t)d * sizeof(double), 256);
}
size_t dcv_spectral_workspace_bytes(int n_tensors, const int32_t* rows, const int32_t* cols) {
    if (!sn_shapes_ok(n_tensors, rows, cols)) { fail(DCV_EINVAL, "spectral_workspace_bytes: bad arguments (rows and cols >= 1, rows * cols <= 2^30)"); return 0; }
    return sn_workspace_bytes(n_tensors, rows, cols);
}

// every tensor's offset into the workspace, in doubles
static std::vector<int64_t> sn_ws_offsets(int n, const int32_t* rows, const int32_t* cols) {
    std::vector<int64_t> off(std::max(n, 1));
    int64_t d = 0;
    for (int t = 0; t < n; ++t) { off[t] = d; d += sn_ws_doubles(rows[t], cols[t]); }
    return off;
}
static void sn_slot_shape(SnPack& k, int t, int M, int K, int64_t ws_off) { k.rows[t] = M; k.cols[t] = K; k.tab.n[t] = (int64_t)M * K; k.ws_off[t] = ws_off; }

int dcv_spectral_update_multi(int n_tensors, const float* const* w, float* const* w_sn, float* const* u, float* const* v, float* const* sigma,
                              const int32_t* rows, const int32_t* cols, int n_iter, double eps, const float* guard_state, void* ws, size_t ws_bytes, void* stream) {
    if (!sn_shapes_ok(n_tensors, rows, cols) || (n_tensors > 0 && (!w || !w_sn || !u || !v || !sigma)) || n_iter < 0 || !(eps > 0.0) || !ws ||
        (reinterpret_cast<uintptr_t>(ws) & 15))
        return fail(DCV_EINVAL, "spectral_update_multi: bad arguments");
    for (int t = 0; t < n_tensors; ++t)
        if (!w[t] || !w_sn[t] || !u[t] || !v[t] || !sigma[t] || w[t] == w_sn[t]) return fail(DCV_EINVAL, "spectral_update_multi: null tensor, or w_sn is w");
    if (sn_workspace_bytes(n_tensors, rows, cols) > ws_bytes) return fail(DCV_EWORKSPACE, "spectral_update_multi: workspace too small");
    hipStream_t s = static_cast<hipStream_t>(stream);
    int32_t* skip = guard_state ? static_cast<int32_t*>(ws) : nullptr;
    double* wsd = reinterpret_cast<double*>(static_cast<char*>(ws) + 256);
    if (guard_state) {
        hipLaunchKernelGGL(sn_prepare_kernel, dim3(1), dim3(1), 0, s, skip, guard_state);
        DCV_LAUNCH_CHECK();
    }
    const std::vector<int64_t> off = sn_ws_offsets(n_tensors, rows, cols);
    // One kernel over every table, then the next kernel (a tensor's kernels still follow each other on the stream; tensors do not depend on each other).
    auto stage = [&](auto kernel, auto blocks_of, int from_prev) {
        return mt_for_tables<SnPack>(n_tensors, [&](int i) { return blocks_of(rows[i], cols[i]); },
            [&](SnPack& k, int t, int i) {
                k.w[t] = w[i]; k.w_sn[t] = w_sn[i]; k.u[t] = u[i]; k.v[t] = v[i]; k.sigma[t] = sigma[i];
                sn_slot_shape(k, t, rows[i], cols[i], off[i]);
            },
            [&](const SnPack& k, int nt, int blocks, int64_t) {
                hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(256), 0, s, k, nt, from_prev, eps, wsd, skip);
                DCV_LAUNCH_CHECK();
                return DCV_OK;
            });
    };
    const auto kchunks = [](int, int K) { return (int64_t)sn_kchunks(K); };
    const auto mchunks = [](int M, int) { return (int64_t)sn_mchunks(M); };
    for (int it = 0; it < n_iter; ++it) {
        if (const int rc = stage(sn_cols_kernel, kchunks, it > 0 ? 1 : 0)) return rc;
        if (const int rc = stage(sn_rows_kernel, mchunks, 1)) return rc;
    }
    if (n_iter == 0)      // sigma of the stored u, v
        if (const int rc = stage(sn_rows_kernel, mchunks, 0)) return rc;
    return stage(sn_scale_kernel, sn_eblocks, n_iter > 0 ? 1 : 0);
}

int dcv_spectral_project_multi(int n_tensors, float* const* g, const float* const* w_sn, const float* const* u, const float* const* v, const float* const* sigma,
                               const int32_t* rows, const int32_t* cols, double eps, void* ws, size_t ws_bytes, void* stream) {
    if (!sn_shapes_ok(n_tensors, rows, cols) || (n_tensors > 0 && (!g || !w_sn || !u || !v || !sigma)) || !(eps > 0.0) || !ws || (reinterpret_cast<uintptr_t>(ws) & 15))
        return fail(DCV_EINVAL, "spectral_project_multi: bad arguments");
    for (int t = 0; t < n_tensors; ++t)
        if (!g[t] || !w_sn[t] || !u[t] || !v[t] || !sigma[t] || g[t] == w_sn[t]) return fail(DCV_EINVAL, "spectral_project_multi: null tensor, or g is w_sn");
    if (sn_workspace_bytes(n_tensors, rows, cols) > ws_bytes) return fail(DCV_EWORKSPACE, "spectral_project_multi: workspace too small");
    hipStream_t s = static_cast<hipStream_t>(stream);
    double* wsd = reinterpret_cast<double*>(static_cast<char*>(ws) + 256);
    const std::vector<int64_t> off = sn_ws_offsets(n_tensors, rows, cols);
    return mt_for_tables<SnPack>(n_tensors, [&](int i) { return sn_eblocks(rows[i], cols[i]); },
        [&](SnPack& k, int t, int i) {
            k.g[t] = g[i]; k.w_sn[t] = const_cast<float*>(w_sn[i]); k.u[t] = const_cast<float*>(u[i]); k.v[t] = const_cast<float*>(v[i]);
            k.sigma[t] = const_cast<float*>(sigma[i]);
            sn_slot_shape(k, t, rows[i], cols[i], off[i]);
        },
        [&](const SnPack& k, int nt, int blocks, int64_t) {
            hipLaunchKernelGGL(sn_inner_kernel, dim3((unsigned)blocks), dim3(256), 0, s, k, nt, wsd);
            DCV_LAUNCH_CHECK();
            hipLaunchKernelGGL(sn_project_kernel, dim3((unsigned)blocks), dim3(256), 0, s, k, nt, eps, wsd);
            DCV_LAUNCH_CHECK();
            return DCV_OK;
        });
}

int dcv_decode_video(const void* in, int in_is_u8, int B, int T, int H, int W, int Cc, float div, float sub, float* out, void* stream) {
    if (!in || !out || B < 1 || T < 1 || H < 1 || W < 1 || Cc < 1 || div == 0.f) return fail(DCV_EINVAL, "decode_video: bad arguments");
    const int64_t total = (int64_t)B * Cc * T * H * W;
    const unsigned grid = (unsigned)((total + 255) / 256);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (in_is_u8) hipLaunchKernelGGL((decode_video_kernel<uint8_t>), dim3(grid), dim3(256), 0, s, static_cast<const uint8_t*>(in), out, (int64_t)T, (int64_t)H * W, Cc, total, div, sub);
    else hipLaunchKernelGGL((decode_video_kernel<float>), dim3(grid), dim3(256), 0, s, static_cast<const float*>(in), out, (int64_t)T, (int64_t)H * W, Cc, total, div, sub);
    DCV_LAUNCH_CHECK();
    return DCV_OK;
}

int dcv_surreal_depth(const float* depth, int B, int T, int H, int W, float* out, float* ws_minmax, void* stream) {
    if (!depth || !out || !ws_minmax || B < 1) return fail(DCV_EINVAL, "surreal_depth: bad arguments");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t per = (int64_t)T * H * W, total = per * B;
    hipLaunchKernelGGL(surreal_minmax_kernel, dim3(B), dim3(256), 0, s, depth, per, ws_minmax);
    DCV_LAUNCH_CHECK();
    hipLaunchKernelGGL(surreal_norm_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, depth, per, total, ws_minmax, out);
    DCV_LAUNCH_CHECK();
    return DCV_OK;
}

static PosView posview(const dcv_dims5& d) { return PosView{d.sn, d.sc, d.sd, d.sh, d.sw, d.c, d.d, d.h, d.w}; }
static bool same_positions(const dcv_dims5& a, const dcv_dims5& b) { return a.n == b.n && a.d == b.d && a.h == b.h && a.w == b.w; }

int dcv_softmax_channels_forward(const float* x, const dcv_dims5* xd, float* y, const dcv_dims5* yd, void* stream) {
    if (!x || !y || !xd || !yd || !same_shape(*xd, *yd) || xd->c < 1) return fail(DCV_EINVAL, "softmax_channels_forward: bad arguments");
    const int64_t P = (int64_t)xd->n * xd->d * xd->h * xd->w;
    hipLaunchKernelGGL(softmax_c_fwd_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), x, posview(*xd), y, posview(*yd), P);
    DCV_LAUNCH_CHECK();
    return DCV_OK;
}

int dcv_softmax_channels_backward(const float* dy, const dcv_dims5* dyd, const float* y, const dcv_dims5* yd, float* dx, const dcv_dims5* dxd, void* stream) {
    if (!dy || !y || !dx || !dyd || !yd || !dxd || !same_shape(*dyd, *yd) || !same_shape(*dyd, *dxd)) return fail(DCV_EINVAL, "softmax_channels_backward: bad arguments");
    const int64_t P = (int64_t)yd->n * yd->d * yd->h * yd->w;
    hipLaunchKernelGGL(softmax_c_bwd_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), dy, posview(*dyd), y, posview(*yd), dx, posview(*dxd), P);
    DCV_LAUNCH_CHECK();
    return DCV_OK;
}

int dcv_segm_onehot(const float* x, const dcv_dims5* xd, float* y, const dcv_dims5* yd, void* stream) {
    if (!x || !y || !xd || !yd || !same_shape(*xd, *yd) || xd->c < 1) return fail(DCV_EINVAL, "segm_onehot: bad arguments");
    const int64_t P = (int64_t)xd->n * xd->d * xd->h * xd->w;
    hipLaunchKernelGGL(segm_onehot_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), x, posview(*xd), y, posview(*yd), P);
    DCV_LAUNCH_CHECK();
    return DCV_OK;
}

int dcv_segm_to_rgb(const float* x, const dcv_dims5* xd, const uint8_t* palette, uint8_t* out, void* stream) {
    if (!x || !xd || !palette || !out || xd->c < 1) return fail(DCV_EINVAL, "segm_to_rgb: bad arguments");
    const int64_t P = (int64_t)xd->n * xd->d * xd->h * xd->w;
    hipLaunchKernelGGL(segm_color_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), x, posview(*xd), palette, out, P);
    DCV_LAUNCH_CHECK();
    return DCV_OK;
}

int dcv_decode_segmentation(const uint8_t* labels, int B, int T, int H, int W, int C, float* out, void* stream) {
    if (!labels || !out || B < 1 || T < 1 || H < 1 || W < 1 || C < 1 || C > 256) return fail(DCV_EINVAL, "decode_segmentation: bad arguments");
    const int64_t per = (int64_t)T * H * W, P = per * B;
    hipLaunchKernelGGL(segm_decode_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), labels, out, C, per, P);
    DCV_LAUNCH_CHECK();
    return DCV_OK;
}

int dcv_videos_to_uint8(const float* x, const dcv_dims5* xd, uint8_t* out, int channel_repeat, void* stream) {
    if (!x || !xd || !out || channel_repeat < 1 || channel_repeat > 4) return fail(DCV_EINVAL, "videos_to_uint8: bad arguments");
    const dcv_dims5* views[1] = {xd};
    const void* ptrs[1] = {x};
    RowMap m = make_rowmap(*xd, views, 1, ptrs);
    ToU8 f{x, out, rv(*xd), channel_repeat};
    return launch_ew(m, f, static_cast<hipStream_t>(stream));
}

int dcv_flow_to_rgb(const float* flow, const dcv_dims5* fd, float scale, uint8_t* out, float* ws_minmax, void* stream) {
    if (!flow || !fd || !out || !ws_minmax || fd->c != 2) return fail(DCV_EINVAL, "flow_to_rgb: needs a (B,2,T,H,W) flow video");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int B = fd->n, T = fd->d, HW = fd->h * fd->w;
    hipLaunchKernelGGL(flow_minmax_kernel, dim3(B * T), dim3(256), 0, s, flow, rv(*fd), T, HW, fd->w, scale, ws_minmax);
    DCV_LAUNCH_CHECK();
    const int64_t tot = (int64_t)B * T * HW;
    hipLaunchKernelGGL(flow_to_rgb_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, flow, rv(*fd), B, T, HW, fd->w, scale, ws_minmax, out);
    DCV_LAUNCH_CHECK();
    return DCV_OK;
}

size_t dcv_gru_workspace_bytes(int B, int dm) { return (size_t)B * (6 * dm * dm + 6 * dm) * sizeof(float) + 256; }

int dcv_gru_forward(const float* e, const float* h0, const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh,
                    float* out, float* gates, int T, int B, int dm, void* stream) {
    if (!e || !h0 || !w_ih || !w_hh || !b_ih || !b_hh || !out || !gates || T < 1 || B < 1 || dm < 1 || dm > GRU_MAXD) return fail(DCV_EINVAL, "gru_forward: bad arguments");
    hipLaunchKernelGGL(gru_fwd_kernel, dim3(B), dim3(64), 0, static_cast<hipStream_t>(stream), e, h0, w_ih, w_hh, b_ih, b_hh, out, gates, T, B, dm);
    DCV_LAUNCH_CHECK();
    return DCV_OK;
}

int dcv_gru_backward(const float* dout, const float* e, const float* h0, const float* out, const float* gates, const float* w_ih, const float* w_hh,
                     float* dw_ih, float* dw_hh, float* db_ih, float* db_hh, int T, int B, int dm, void* ws, size_t ws_bytes, void* stream) {
    (void)w_ih;
    if (!dout || !e || !h0 || !out || !gates || !w_hh || !dw_ih || !dw_hh || !db_ih || !db_hh || T < 1 || B < 1 || dm < 1 || dm > GRU_MAXD) return fail(DCV_EINVAL, "gru_backward: bad arguments");
    if (!ws || ws_bytes < dcv_gru_workspace_bytes(B, dm)) return fail(DCV_EWORKSPACE, "gru_backward: workspace too small");
    hipStream_t s = static_cast<hipStream_t>(stream);
    float* part = static_cast<float*>(ws);
    const int P = 6 * dm * dm + 6 * dm;
    const int lds_acc = (size_t)P * sizeof(float) <= 48 * 1024;   // dm <= 44: the partial sums live in LDS
    hipLaunchKernelGGL(gru_bwd_kernel, dim3(B), dim3(64), lds_acc ? (size_t)P * sizeof(float) : 0, s, dout, e, h0, out, gates, w_hh, part, T, B, dm, lds_acc);
    DCV_LAUNCH_CHECK();
    hipLaunchKernelGGL(gru_reduce_kernel, dim3((P + 255) / 256), dim3(256), 0, s, part, B, P, dm, dw_ih, dw_hh, db_ih, db_hh);
    DCV_LAUNCH_CHECK();
    return DCV_OK;
}

}  // extern "C"
