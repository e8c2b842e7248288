// The device-resident dataset, gfx950: every video's decoded frames stay in HBM, back to back in disk order, and a training batch is made from them on
// the device.  clip_draw_kernel writes a (B, 2) int32 table (clip, t0) — the epoch's shuffle and the reference's random window (dataset.py:116-123, train.py:101-109) —
// and one gather launch per stream turns the table into the normalised fp32 (B, C, T, H, W) batch with the arithmetic of the batch decoders (dcv_common.h), so the
// bytes are those of dataprep.decode_* on the same frames.  No atomics, no state: a table row depends on (seed, epoch, position) alone.
#include "dcv_common.h"

namespace dcv {

// ---- the draw ------------------------------------------------------------------------------------------------------------------------------------------------
// clip = clip_perm(position) under (seed, epoch): the keyed bijection on [0, N) of dcv_common.h (the kernel distance draws its subsets with it too).
// One thread per row.  The window start of a video of n > T frames is mulhi32(u, n - T) in [0, n - T - 1] (np.random.randint(n - T) of dataset.py:122: the last
// window is never drawn), u = word 0 of Philox with counter {position, 0xFFFFFFFF, epoch lo, epoch hi}: no Feistel round has that counter (r < 2^32 - 1).
__global__ __launch_bounds__(64) void clip_draw_kernel(int32_t* __restrict__ table, int B, const int64_t* __restrict__ starts, uint32_t N, int T, int h, uint32_t k0,
                                                       uint32_t k1, uint32_t e0, uint32_t e1, uint32_t first_position) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const uint32_t pos = first_position + (uint32_t)b;
    const uint32_t clip = clip_perm(pos, N, h, k0, k1, e0, e1);
    const int64_t n = starts[clip + 1] - starts[clip];
    uint32_t c[4] = {pos, 0xFFFFFFFFu, e0, e1};
    philox4x32_10(c, k0, k1);
    const int32_t t0 = n > (int64_t)T ? (int32_t)__umulhi(c[0], (uint32_t)(n - T)) : 0;
    table[2 * b] = (int32_t)clip;
    table[2 * b + 1] = t0;
}

// ---- the gather ----------------------------------------------------------------------------------------------------------------------------------------------
// A clip's window is T consecutive frames = ONE contiguous run of L = T*H*W pixels of C interleaved values, and plane (b, c) of the output is L consecutive
// floats: the gather is a per-clip de-interleave.  A thread owns four consecutive pixels: it reads 4*C*sizeof(TIN) contiguous bytes (a wave: one contiguous run)
// and writes one float4 per channel (a wave: 1 KiB contiguous per channel).

// The first frame of row b's window, or -1 if the row does not name T frames of one video (a drawn table always does; the Python layer refuses an injected one
// that does not, and a row that is wrong all the same is written as NaN / zeros instead of being read out of bounds).
__device__ __forceinline__ int64_t clip_first_frame(const int32_t* __restrict__ table, const int64_t* __restrict__ starts, int N, int T, int b) {
    const int32_t clip = table[2 * b], t0 = table[2 * b + 1];
    if (clip < 0 || clip >= N || t0 < 0) return -1;
    const int64_t s = starts[clip];
    if ((int64_t)t0 + T > starts[clip + 1] - s) return -1;
    return s + t0;
}

// NB contiguous bytes at s -> words.  The widest load the ADDRESS allows: a window starts at frame * H*W*C bytes, which for H*W*C not a multiple of 16 (or of 4)
// is on no 16-byte (4-byte) boundary, so the choice is made per access, from the address.
template <int NB>
__device__ __forceinline__ void clip_load(const uint8_t* __restrict__ s, uint32_t (&w)[NB / 4]) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(s);
    if (NB % 16 == 0 && a % 16 == 0) {
#pragma unroll
        for (int i = 0; i < NB / 16; ++i) __builtin_memcpy(&w[4 * i], __builtin_assume_aligned(s + 16 * i, 16), 16);
    } else if (a % 4 == 0) {
#pragma unroll
        for (int i = 0; i < NB / 4; ++i) __builtin_memcpy(&w[i], __builtin_assume_aligned(s + 4 * i, 4), 4);
    } else {
#pragma unroll
        for (int i = 0; i < NB / 4; ++i)
            w[i] = (uint32_t)s[4 * i] | ((uint32_t)s[4 * i + 1] << 8) | ((uint32_t)s[4 * i + 2] << 16) | ((uint32_t)s[4 * i + 3] << 24);
    }
}
__device__ __forceinline__ float clip_elem(const uint32_t* w, int k, uint8_t) { return (float)((w[k >> 2] >> (8 * (k & 3))) & 0xffu); }
__device__ __forceinline__ float clip_elem(const uint32_t* w, int k, float) { return __builtin_bit_cast(float, w[k]); }

typedef float clip_f4 __attribute__((ext_vector_type(4)));

// out[b][c][p] = decode_value(src[(first_frame * HW + p) * CC + c]): uint8 or fp32 frames (F, H, W, CC)
template <class TIN, int CC>
__global__ __launch_bounds__(256) void clip_gather_kernel(const TIN* __restrict__ src, const int32_t* __restrict__ table, const int64_t* __restrict__ starts, int N,
                                                          int T, int64_t HW, float div, float sub, float* __restrict__ out, int vec_store) {
    const int b = blockIdx.y;
    const int64_t L = (int64_t)T * HW;
    const int64_t p0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (p0 >= L) return;
    const int n = L - p0 < 4 ? (int)(L - p0) : 4;
    float* o = out + (int64_t)b * CC * L + p0;
    const int64_t f0 = clip_first_frame(table, starts, N, T, b);
    float r[CC][4];
    if (f0 < 0) {
#pragma unroll
        for (int c = 0; c < CC; ++c)
#pragma unroll
            for (int j = 0; j < 4; ++j) r[c][j] = __builtin_nanf("");
    } else {
        const TIN* s = src + (f0 * HW + p0) * CC;      // 64-bit: a store is far beyond 2^31 bytes
        constexpr int NB = 4 * CC * (int)sizeof(TIN);
        uint32_t w[NB / 4];
        if (n == 4) {
            clip_load<NB>(reinterpret_cast<const uint8_t*>(s), w);
#pragma unroll
            for (int c = 0; c < CC; ++c)
#pragma unroll
                for (int j = 0; j < 4; ++j) r[c][j] = decode_value(clip_elem(w, j * CC + c, TIN()), div, sub);
        } else {      // the last pixels of a window whose length is no multiple of four
#pragma unroll
            for (int c = 0; c < CC; ++c)
#pragma unroll
                for (int j = 0; j < 4; ++j) r[c][j] = j < n ? decode_value((float)s[j * CC + c], div, sub) : 0.f;
        }
    }
    if (vec_store && n == 4) {      // L % 4 == 0 and `out` on a 16-byte boundary: every plane's quad is
#pragma unroll
        for (int c = 0; c < CC; ++c) *reinterpret_cast<clip_f4*>(o + c * L) = clip_f4{r[c][0], r[c][1], r[c][2], r[c][3]};
    } else {
#pragma unroll
        for (int c = 0; c < CC; ++c)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < n) o[c * L + j] = r[c][j];
    }
}

// out[b][c][p] = onehot_value(labels[first_frame * HW + p], c): uint8 label frames (F, H, W) -> C one-hot planes (dataset.py:176-181)
__global__ __launch_bounds__(256) void clip_onehot_kernel(const uint8_t* __restrict__ src, const int32_t* __restrict__ table, const int64_t* __restrict__ starts, int N,
                                                          int T, int64_t HW, int C, float* __restrict__ out, int vec_store) {
    const int b = blockIdx.y;
    const int64_t L = (int64_t)T * HW;
    const int64_t p0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (p0 >= L) return;
    const int n = L - p0 < 4 ? (int)(L - p0) : 4;
    float* o = out + (int64_t)b * C * L + p0;
    const int64_t f0 = clip_first_frame(table, starts, N, T, b);
    int l[4] = {-1, -1, -1, -1};      // a refused row: all-zero planes
    if (f0 >= 0) {
        const uint8_t* s = src + f0 * HW + p0;
        if (n == 4) {
            uint32_t w[1];
            clip_load<4>(s, w);
#pragma unroll
            for (int j = 0; j < 4; ++j) l[j] = (int)((w[0] >> (8 * j)) & 0xffu);
        } else {
            for (int j = 0; j < n; ++j) l[j] = s[j];
        }
    }
    if (vec_store && n == 4) {
        for (int c = 0; c < C; ++c)
            *reinterpret_cast<clip_f4*>(o + c * L) = clip_f4{onehot_value(l[0], c), onehot_value(l[1], c), onehot_value(l[2], c), onehot_value(l[3], c)};
    } else {
        for (int c = 0; c < C; ++c)
            for (int j = 0; j < n; ++j) o[c * L + j] = onehot_value(l[j], c);
    }
}

// SURREAL depth (dataset.py:136-156), in place on the gathered raw window: one workgroup per clip finds the foreground's min and max over the WINDOW, then
// normalises it with the arithmetic of dcv_surreal_depth.  min / max do not depend on the order they are taken in.
__global__ __launch_bounds__(1024) void clip_surreal_kernel(float* x, int64_t per_clip) {
    __shared__ float smin[16], smax[16];
    float* p = x + (int64_t)blockIdx.x * per_clip;
    float lo = 3.4e38f, hi = -3.4e38f;
    for (int64_t i = threadIdx.x; i < per_clip; i += 1024) surreal_fold(p[i], lo, hi);
    for (int o = 32; o > 0; o >>= 1) { lo = fminf(lo, __shfl_xor(lo, o, 64)); hi = fmaxf(hi, __shfl_xor(hi, o, 64)); }
    if ((threadIdx.x & 63) == 0) { smin[threadIdx.x >> 6] = lo; smax[threadIdx.x >> 6] = hi; }
    __syncthreads();      // every lane has read its raw values; the writes below touch the lane's own elements only
    lo = smin[0]; hi = smax[0];
#pragma unroll
    for (int k = 1; k < 16; ++k) { lo = fminf(lo, smin[k]); hi = fmaxf(hi, smax[k]); }
    for (int64_t i = threadIdx.x; i < per_clip; i += 1024) p[i] = surreal_value(p[i], lo, hi);
}

template <class TIN>
static void clip_gather_launch(int C, dim3 grid, hipStream_t s, const void* frames, const int32_t* table, const int64_t* starts, int N, int T, int64_t HW, float div,
                               float sub, float* out, int vec) {
    const TIN* f = static_cast<const TIN*>(frames);
    switch (C) {
        case 1: hipLaunchKernelGGL((clip_gather_kernel<TIN, 1>), grid, dim3(256), 0, s, f, table, starts, N, T, HW, div, sub, out, vec); break;
        case 2: hipLaunchKernelGGL((clip_gather_kernel<TIN, 2>), grid, dim3(256), 0, s, f, table, starts, N, T, HW, div, sub, out, vec); break;
        case 3: hipLaunchKernelGGL((clip_gather_kernel<TIN, 3>), grid, dim3(256), 0, s, f, table, starts, N, T, HW, div, sub, out, vec); break;
        default: hipLaunchKernelGGL((clip_gather_kernel<TIN, 4>), grid, dim3(256), 0, s, f, table, starts, N, T, HW, div, sub, out, vec); break;
    }
}

}  // namespace dcv

using namespace dcv;

extern "C" {

int dcv_clipstore_draw(int32_t* table, int B, const int64_t* starts, int64_t N, int T, uint64_t seed, uint64_t epoch, int64_t first_position, void* stream) {
    if (!table || !starts || reinterpret_cast<uintptr_t>(table) % 4 || reinterpret_cast<uintptr_t>(starts) % 8)
        return fail(DCV_EINVAL, "clipstore_draw: null or misaligned table / starts");
    if (B < 1 || T < 1 || N < 1 || N > 0x7fffffffll) return fail(DCV_EINVAL, "clipstore_draw: B >= 1, T >= 1, 1 <= N < 2^31 (got B %d, T %d, N %lld)", B, T, (long long)N);
    if (first_position < 0 || first_position + B > N)
        return fail(DCV_EINVAL, "clipstore_draw: positions %lld .. %lld are not inside the epoch's [0, %lld)", (long long)first_position, (long long)first_position + B - 1,
                    (long long)N);
    hipLaunchKernelGGL(clip_draw_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, static_cast<hipStream_t>(stream), table, B, starts, (uint32_t)N, T, clip_perm_half_bits(N),
                       (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)epoch, (uint32_t)(epoch >> 32), (uint32_t)first_position);
    DCV_LAUNCH_CHECK();
    return DCV_OK;
}

int dcv_clipstore_gather(const void* frames, int mode, const int32_t* table, const int64_t* starts, int64_t N, int B, int T, int H, int W, int C, float div, float sub,
                         float* out, void* stream) {
    if (!frames || !table || !starts || !out || reinterpret_cast<uintptr_t>(table) % 4 || reinterpret_cast<uintptr_t>(starts) % 8 || reinterpret_cast<uintptr_t>(out) % 4)
        return fail(DCV_EINVAL, "clipstore_gather: null or misaligned pointer");
    if (mode == DCV_CLIP_F32 && reinterpret_cast<uintptr_t>(frames) % 4) return fail(DCV_EINVAL, "clipstore_gather: fp32 frames on no 4-byte boundary");
    if (B < 1 || B > 65535 || T < 1 || H < 1 || W < 1 || N < 1 || N > 0x7fffffffll)
        return fail(DCV_EINVAL, "clipstore_gather: 1 <= B <= 65535, T, H, W >= 1, 1 <= N < 2^31 (got B %d, T %d, H %d, W %d, N %lld)", B, T, H, W, (long long)N);
    const int64_t HW = (int64_t)H * W, L = HW * T, quads = (L + 3) / 4;
    if ((quads + 255) / 256 > 0x7fffffffll) return fail(DCV_EINVAL, "clipstore_gather: a clip of %lld pixels is too large", (long long)L);
    const dim3 grid((unsigned)((quads + 255) / 256), (unsigned)B);
    const int vec = (L % 4 == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0) ? 1 : 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (mode == DCV_CLIP_LABELS) {
        if (C < 1 || C > 256) return fail(DCV_EINVAL, "clipstore_gather: 1 <= C <= 256 one-hot parts (got %d)", C);
        hipLaunchKernelGGL(clip_onehot_kernel, grid, dim3(256), 0, s, static_cast<const uint8_t*>(frames), table, starts, (int)N, T, HW, C, out, vec);
    } else if (mode == DCV_CLIP_U8 || mode == DCV_CLIP_F32) {
        if (C < 1 || C > 4 || div == 0.f) return fail(DCV_EINVAL, "clipstore_gather: 1 <= C <= 4 interleaved channels and div != 0 (got C %d, div %g)", C, (double)div);
        if (mode == DCV_CLIP_U8) clip_gather_launch<uint8_t>(C, grid, s, frames, table, starts, (int)N, T, HW, div, sub, out, vec);
        else clip_gather_launch<float>(C, grid, s, frames, table, starts, (int)N, T, HW, div, sub, out, vec);
    } else {
        return fail(DCV_EINVAL, "clipstore_gather: unknown mode %d", mode);
    }
    DCV_LAUNCH_CHECK();
    return DCV_OK;
}

int dcv_clipstore_surreal(float* clips, int B, int64_t per_clip, void* stream) {
    if (!clips || reinterpret_cast<uintptr_t>(clips) % 4 || B < 1 || per_clip < 1) return fail(DCV_EINVAL, "clipstore_surreal: bad arguments");
    hipLaunchKernelGGL(clip_surreal_kernel, dim3((unsigned)B), dim3(1024), 0, static_cast<hipStream_t>(stream), clips, per_clip);
    DCV_LAUNCH_CHECK();
    return DCV_OK;
}

}  // extern "C"
