// Internal helpers shared by the gfx950 kernel translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "dcvgan_hip.h"

namespace dcv {

extern thread_local char g_err[512];
extern std::atomic<uint64_t> g_launches;

inline int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

#define DCV_HIP_CHECK(expr)                                                              \
    do {                                                                                 \
        hipError_t e_ = (expr);                                                          \
        if (e_ != hipSuccess)                                                            \
            return dcv::fail(DCV_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

#define DCV_LAUNCH_CHECK()                                                               \
    do {                                                                                 \
        dcv::g_launches.fetch_add(1, std::memory_order_relaxed);                         \
        hipError_t e_ = hipGetLastError();                                               \
        if (e_ != hipSuccess)                                                            \
            return dcv::fail(DCV_EHIP, "kernel launch failed: %s (%s:%d)", hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

inline int64_t numel(const dcv_dims5& d) { return (int64_t)d.n * d.c * d.d * d.h * d.w; }
inline bool same_shape(const dcv_dims5& a, const dcv_dims5& b) {
    return a.n == b.n && a.c == b.c && a.d == b.d && a.h == b.h && a.w == b.w;
}
inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// 32-bit magic division (exact for all 0 <= n < 2^31 with 1 <= d < 2^31):
// q = (uint64(n) * mul) >> 32 >> shift
struct FastDiv {
    uint32_t mul, shift, div, pad;
};
inline FastDiv make_fastdiv(uint32_t d) {
    FastDiv f;
    f.div = d;
    f.pad = 0;
    if (d == 1) { f.mul = 0; f.shift = 0; return f; }
    uint32_t l = 0;
    while ((1ull << l) < d) ++l;   // ceil(log2 d)
    uint64_t m = ((1ull << 32) * ((1ull << l) - d)) / d + 1;
    f.mul = (uint32_t)m;
    f.shift = l;
    return f;
}

}  // namespace dcv

#ifdef __HIPCC__
// Element type of the 16-bit channels-last path (conv_cl16.hip, cl_elementwise.hip): bf16 by default; -DDCV_CL_FP16 compiles the same two translation units a second
// time for fp16 — same MFMA rate and fragment path (v_mfma_f32_32x32x16_f16), 10 mantissa bits instead of 7, exponent range 6.5e4 instead of fp32's — with the entry
// points renamed dcv_cl_* -> dcv_clf16_* (BASELINE configs[4] names fp16 MFMA; built for the discriminators' stress shape).
namespace dcv {
#ifdef DCV_CL_FP16
typedef _Float16 cl_h;
#define CL_MFMA __builtin_amdgcn_mfma_f32_32x32x16_f16
#define CL_HALF_NAME "fp16"
#else
typedef __bf16 cl_h;
#define CL_MFMA __builtin_amdgcn_mfma_f32_32x32x16_bf16
#define CL_HALF_NAME "bf16"
#endif
typedef cl_h cl_h8 __attribute__((ext_vector_type(8)));
typedef cl_h cl_h2 __attribute__((ext_vector_type(2)));
// two floats -> one dword of two 16-bit values (round to nearest even), and back
__device__ __forceinline__ uint32_t cl_pack2(float a, float b) {
    typedef float f32x2c __attribute__((ext_vector_type(2)));
    const f32x2c t = {a, b};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(t, cl_h2));
}
#ifdef DCV_CL_FP16
__device__ __forceinline__ float cl_lo(uint32_t w) { return (float)__builtin_bit_cast(cl_h2, w)[0]; }
__device__ __forceinline__ float cl_hi(uint32_t w) { return (float)__builtin_bit_cast(cl_h2, w)[1]; }
#else
__device__ __forceinline__ float cl_lo(uint32_t w) { return __builtin_bit_cast(float, w << 16); }
__device__ __forceinline__ float cl_hi(uint32_t w) { return __builtin_bit_cast(float, w & 0xffff0000u); }
#endif
__device__ __forceinline__ float cl_round(float v) { return (float)(cl_h)v; }      // the value as it will be stored
}  // namespace dcv
namespace dcv {
// Philox4x32-10 (Salmon et al. 2011): counter c, key (k0, k1); every random draw of the library (elementwise.hip, augment.hip)
__device__ __forceinline__ void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c[0]), lo0 = 0xD2511F53u * c[0];
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c[2]), lo1 = 0xCD9E8D57u * c[2];
        const uint32_t n0 = hi1 ^ c[1] ^ k0, n1 = lo1, n2 = hi0 ^ c[3] ^ k1, n3 = lo0;
        c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}
}  // namespace dcv
namespace dcv {
// The keyed bijection of the library's shuffles (clipstore.hip: the epoch's order; evalstats.hip: the kernel distance's subsets).
static const int CLIP_FEISTEL_ROUNDS = 8;
// perm(seed, epoch, .): a keyed bijection on [0, N).  A balanced Feistel network on w = 2 h bits (the smallest even width with 2^w >= N, at least 2) is a bijection
// on [0, 2^w) whatever its round function is; walking its cycle until the value is below N restricts it to [0, N) (Black & Rogaway 2002).  2^w < 4 N, so the walk
// takes fewer than four network passes on average.  Round r maps (L, R) to (R, L ^ F_r(R)), F_r(R) = the low h bits of word 0 of Philox4x32-10 with counter
// {R, r, epoch lo, epoch hi} and key (seed lo, seed hi).
__device__ __forceinline__ uint32_t clip_perm(uint32_t x, uint32_t N, int h, uint32_t k0, uint32_t k1, uint32_t e0, uint32_t e1) {
    const uint32_t mask = (1u << h) - 1u;
    do {
        uint32_t L = x >> h, R = x & mask;
        for (int r = 0; r < CLIP_FEISTEL_ROUNDS; ++r) {
            uint32_t c[4] = {R, (uint32_t)r, e0, e1};
            philox4x32_10(c, k0, k1);
            const uint32_t t = L ^ (c[0] & mask);
            L = R; R = t;
        }
        x = (L << h) | R;
    } while (x >= N);
    return x;
}
// h of clip_perm for [0, N): half the smallest even width that covers it, at least 1
inline int clip_perm_half_bits(int64_t N) {
    int bits = 0;
    while ((1ll << bits) < N) ++bits;
    const int w = bits + (bits & 1) < 2 ? 2 : bits + (bits & 1);
    return w / 2;
}
}  // namespace dcv
namespace dcv {
// The input pipeline's per-element arithmetic (dataset.py:125-181), shared by the batch decoders (elementwise.hip) and the clip store's gather (clipstore.hip): one
// definition, so a gathered batch holds the bytes the decoders write.  numpy's fp32 operation order, every operation rounded on its own.
__device__ __forceinline__ float decode_value(float v, float div, float sub) {      // dataset.py:131, 168, 174
#pragma clang fp contract(off)
    return v / div - sub;
}
__device__ __forceinline__ float onehot_value(int label, int c) { return c == label ? 1.f : 0.f; }      // dataset.py:180
// SURREAL depth (dataset.py:137-156): foreground = depth < 1e10; its min and max start at +-3.4e38
__device__ __forceinline__ void surreal_fold(float v, float& lo, float& hi) {
    if (v < 1e10f) { lo = fminf(lo, v); hi = fmaxf(hi, v); }
}
__device__ __forceinline__ float surreal_value(float v, float mi, float ma) {
#pragma clang fp contract(off)   // numpy rounds h*1.8 before subtracting; no fma
    float o = 1.0f;                                        // background
    if (v < 1e10f) {
        float h = v;
        if (ma - mi > 0.f) h = (v - mi) / (ma - mi);
        o = h * 1.8f - 1.0f;                               // [-1.0, 0.8]
    }
    return o;
}
}  // namespace dcv
namespace dcv {
// The fp64 matrix pipe and the 256-lane tree of the evaluation kernels (evalstats.hip: moments and kernel distance; evalknn.hip: the k-nearest-neighbour metrics).
typedef double ev_d4 __attribute__((ext_vector_type(4)));
typedef float ev_f4 __attribute__((ext_vector_type(4)));

// v_mfma_f64_16x16x4_f64: D = A (16 x 4) * B (4 x 16) + C.  Lane l holds A[row l & 15][k = l >> 4] and B[k = l >> 4][col l & 15], one double each, and
// C/D[row (l >> 4) + 4 r][col l & 15] in element r of its four: NOT the row map of the other MFMA forms (4 (l >> 4) + r).
__device__ __forceinline__ ev_d4 ev_mfma(double a, double b, ev_d4 c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }

// The order above the lanes, as lecam.hip has it: p[l] += p[l + s] for s = 128 .. 1; every lane returns p[0].
__device__ __forceinline__ double ev_tree_sum(double v, double* p) {
    const int l = threadIdx.x;
    __syncthreads();      // the previous tree's p[0] has been read by every lane
    p[l] = v;
    __syncthreads();
#pragma unroll
    for (int s = 128; s >= 1; s >>= 1) {
        if (l < s) p[l] += p[l + s];
        __syncthreads();
    }
    return p[0];
}
}  // namespace dcv
namespace dcv {
// n / d for the FastDiv above (d == 1 handled by mul == 0 convention)
__device__ __forceinline__ uint32_t fdiv(uint32_t n, const FastDiv f) {
    if (f.div == 1) return n;
    uint32_t t = __umulhi(n, f.mul);
    return (t + ((n - t) >> 1)) >> (f.shift - 1);
}
}  // namespace dcv
#endif
