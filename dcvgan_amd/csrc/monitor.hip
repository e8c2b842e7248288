// RunMonitor, gfx950: the training log kept on the device.  dcv_monitor_observe folds one iteration's fp32 scalars (losses, gradient norms, LeCam terms)
// and logit tensors into a window of 8-byte words, dcv_monitor_roll publishes the window into a caller-given record and resets it; dcv_hist_u8 and
// dcv_video_grid_u8 are the sample log's histogram and mosaic.  The floating-point sums have ONE fixed order (256 lanes, then an LDS tree, as lecam.hip) and no
// atomics: the same inputs give the same bits.  Only the histogram uses atomics, on integers, where the order of addition does not matter.
// monitor.monitor_host / hist_host / grid_host are the numpy mirrors.
#include "dcv_common.h"

namespace dcv {

// Every operation of this file is rounded on its own, never fused into a multiply-add (the mirror is sum, round, add, round).
#pragma clang fp contract(off)

static const int64_t MON_MAX_N = 1 << 24;
static const int MON_H = DCV_MONITOR_HEADER_WORDS, MON_SW = DCV_MONITOR_SLOT_WORDS, MON_GW = DCV_MONITOR_GROUP_WORDS;
static const uint64_t MON_POS_INF = 0x7FF0000000000000ull, MON_NEG_INF = 0xFFF0000000000000ull;

struct MonArgs {      // the caller's host tables, by value
    const float* slot[DCV_MONITOR_MAX_SLOTS];
    const float* group[DCV_MONITOR_MAX_GROUPS];
    int32_t n[DCV_MONITOR_MAX_GROUPS];
    int32_t n_slots, n_groups;
};

__device__ __forceinline__ double mon_f64(int64_t w) { return __builtin_bit_cast(double, w); }
__device__ __forceinline__ int64_t mon_i64(double v) { return __builtin_bit_cast(int64_t, v); }

// The normative order above the lanes: p[l] += p[l + s] for s = 128 .. 1; every lane returns p[0].  A step's readers (l + s >= s) are not its writers (l < s).
template <class T>
__device__ __forceinline__ T mon_tree(T v, T* p) {
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

// Block g < n_groups: logit group g; block n_groups: the scalars (lane s owns slot s) and the header's observation count.
__global__ __launch_bounds__(256) void monitor_observe_kernel(MonArgs a, int64_t* __restrict__ state) {
    __shared__ double pd[256];
    __shared__ long long pi[256];
    const int g = blockIdx.x, l = threadIdx.x;
    if (g == a.n_groups) {
        if (l == 0) state[DCV_MONITOR_OBSERVATIONS] += 1;
        if (l >= a.n_slots || !a.slot[l]) return;      // a null slot was not observed this iteration
        int64_t* w = state + MON_H + l * MON_SW;
        const float v = *a.slot[l];
        const double d = (double)v;
        w[DCV_MONITOR_SLOT_LAST] = mon_i64(d);
        if (__builtin_isfinite(v)) {
            w[DCV_MONITOR_SLOT_SUM] = mon_i64(mon_f64(w[DCV_MONITOR_SLOT_SUM]) + d);
            w[DCV_MONITOR_SLOT_COUNT] += 1;
            if (d < mon_f64(w[DCV_MONITOR_SLOT_MIN])) w[DCV_MONITOR_SLOT_MIN] = mon_i64(d);
            if (d > mon_f64(w[DCV_MONITOR_SLOT_MAX])) w[DCV_MONITOR_SLOT_MAX] = mon_i64(d);
        } else {
            w[DCV_MONITOR_SLOT_NONFINITE] += 1;
        }
        return;
    }
    const float* __restrict__ y = a.group[g];
    if (!y) return;      // a null group is skipped (uniform over the block: no barrier is left behind)
    const int n = a.n[g];
    double s = 0.0, q = 0.0;
    long long pos = 0, neg = 0, bad = 0;
    for (int i = l; i < n; i += 256) {
        const float v = y[i];
        if (__builtin_isfinite(v)) {
            const double d = (double)v;
            const double dd = d * d;
            s += d;
            q += dd;
            pos += v > 0.f ? 1 : 0;
            neg += v < 0.f ? 1 : 0;
        } else {
            bad += 1;
        }
    }
    const double S = mon_tree(s, pd);
    const double Q = mon_tree(q, pd);
    const long long P = mon_tree(pos, pi), Ng = mon_tree(neg, pi), B = mon_tree(bad, pi);
    if (l != 0) return;
    int64_t* w = state + MON_H + a.n_slots * MON_SW + g * MON_GW;
    w[DCV_MONITOR_GROUP_N] += n;
    w[DCV_MONITOR_GROUP_SUM] = mon_i64(mon_f64(w[DCV_MONITOR_GROUP_SUM]) + S);
    w[DCV_MONITOR_GROUP_SUMSQ] = mon_i64(mon_f64(w[DCV_MONITOR_GROUP_SUMSQ]) + Q);
    w[DCV_MONITOR_GROUP_POS] += P;
    w[DCV_MONITOR_GROUP_NEG] += Ng;
    w[DCV_MONITOR_GROUP_NONFINITE] += B;
}

// One workgroup; every word has one owner, which reads it, publishes it and resets it.
__global__ __launch_bounds__(256) void monitor_roll_kernel(int n_slots, int n_groups, int64_t* __restrict__ state, int64_t* __restrict__ record, int64_t iteration) {
    const int total = MON_H + n_slots * MON_SW + n_groups * MON_GW;
    for (int i = threadIdx.x; i < total; i += 256) {
        const int64_t v = state[i];
        int64_t pub = v, next = 0;
        if (i < MON_H) {
            if (i == DCV_MONITOR_FIRST_ITERATION) next = iteration + 1;
            if (i == DCV_MONITOR_LAST_ITERATION) { pub = iteration; next = iteration; }
            if (i == DCV_MONITOR_ROLLS) next = v + 1;
        } else if (i < MON_H + n_slots * MON_SW) {
            const int f = (i - MON_H) % MON_SW;
            if (f == DCV_MONITOR_SLOT_MIN) next = (int64_t)MON_POS_INF;
            if (f == DCV_MONITOR_SLOT_MAX) next = (int64_t)MON_NEG_INF;
        }
        record[i] = pub;
        state[i] = next;
    }
}

// ---- the sample log's histogram ---------------------------------------------------------------------------------------------------------------------------------
// A workgroup takes (at most) HIST_CHUNK bytes of one clip's run of channel `channel` (T*H*W contiguous bytes).  Counters are privatised in LDS: HIST_COPIES tables
// of 256 32-bit bins per wave (a lane adds into table lane & (HIST_COPIES - 1) of its wave), and a lane first folds the equal neighbours among its 16 bytes into
// one add: a depth clip's background puts whole vectors into one bin, and it is the adds to one LDS address that serialise.  The chunk's bytes before the first
// and after the last 16-byte boundary go one byte per lane.
static const int HIST_CHUNK = 16384, HIST_COPIES = 4, HIST_TABLES = 4 * HIST_COPIES;

__global__ __launch_bounds__(256) void hist_zero_kernel(unsigned long long* __restrict__ counts) { counts[threadIdx.x] = 0ull; }

__global__ __launch_bounds__(256) void hist_u8_kernel(const uint8_t* __restrict__ x, int64_t run, int64_t clip_stride, int chunks, unsigned long long* __restrict__ counts) {
    __shared__ uint32_t bins[HIST_TABLES][256];
    const int l = threadIdx.x;
    for (int i = l; i < HIST_TABLES * 256; i += 256) (&bins[0][0])[i] = 0u;
    __syncthreads();
    const int64_t clip = blockIdx.x / chunks, chunk = blockIdx.x % chunks;
    const int64_t lo = chunk * HIST_CHUNK, hi = lo + HIST_CHUNK < run ? lo + HIST_CHUNK : run;
    const uint8_t* p0 = x + clip * clip_stride + lo;
    const uint8_t* p1 = x + clip * clip_stride + hi;
    uint32_t* mine = bins[(l >> 6) * HIST_COPIES + (l & (HIST_COPIES - 1))];
    // [p0, a0) head, [a0, a1) 16-byte vectors, [a1, p1) tail
    const uintptr_t u0 = reinterpret_cast<uintptr_t>(p0), u1 = reinterpret_cast<uintptr_t>(p1);
    uintptr_t a0 = (u0 + 15) & ~(uintptr_t)15;
    if (a0 > u1) a0 = u1;
    uintptr_t a1 = u1 & ~(uintptr_t)15;
    if (a1 < a0) a1 = a0;
    if ((uintptr_t)l < a0 - u0) atomicAdd(&mine[p0[l]], 1u);
    if ((uintptr_t)l < u1 - a1) atomicAdd(&mine[reinterpret_cast<const uint8_t*>(a1)[l]], 1u);
    const uint4* v = reinterpret_cast<const uint4*>(a0);
    const int nv = (int)((a1 - a0) >> 4);
    for (int i = l; i < nv; i += 256) {
        const uint4 q = v[i];
        const uint32_t w[4] = {q.x, q.y, q.z, q.w};
        uint32_t cur = w[0] & 255u, cnt = 0;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const uint32_t b = (w[k >> 2] >> (8 * (k & 3))) & 255u;
            if (b != cur) { atomicAdd(&mine[cur], cnt); cur = b; cnt = 0; }
            cnt += 1;
        }
        atomicAdd(&mine[cur], cnt);
    }
    __syncthreads();
    unsigned long long t = 0;
#pragma unroll
    for (int k = 0; k < HIST_TABLES; ++k) t += bins[k][l];
    if (t) atomicAdd(&counts[l], t);
}

// ---- the sample log's mosaic ------------------------------------------------------------------------------------------------------------------------------------
// out (T, 3, rows*H, 2*cols*W): row (t, ch, r*H + h) = the W-byte rows (clip r*cols + c, ch, t, h) of `geo` for c = 0 .. cols-1, then those of `colour`.
// One thread per unit of U bytes (16, or 1): a pure gather.
template <class U>
__global__ __launch_bounds__(256) void video_grid_kernel(const U* __restrict__ geo, const U* __restrict__ colour, int rows, int cols, int T, int H, int Wu, int64_t units,
                                                         U* __restrict__ out) {
    const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (u >= units) return;
    int64_t r = u;
    const int wu = (int)(r % Wu); r /= Wu;
    const int c = (int)(r % cols); r /= cols;
    const int side = (int)(r % 2); r /= 2;
    const int h = (int)(r % H); r /= H;
    const int gr = (int)(r % rows); r /= rows;
    const int ch = (int)(r % 3); r /= 3;
    const int t = (int)r;
    const int64_t clip = (int64_t)gr * cols + c;
    const int64_t src = ((((clip * 3 + ch) * T + t) * H + h) * (int64_t)Wu) + wu;
    out[u] = (side ? colour : geo)[src];
}

static int mon_check_state(const char* who, int n_slots, int n_groups, const void* state) {
    if (n_slots < 0 || n_slots > DCV_MONITOR_MAX_SLOTS) return fail(DCV_EINVAL, "%s: 0 <= n_slots <= %d (got %d)", who, DCV_MONITOR_MAX_SLOTS, n_slots);
    if (n_groups < 0 || n_groups > DCV_MONITOR_MAX_GROUPS) return fail(DCV_EINVAL, "%s: 0 <= n_groups <= %d (got %d)", who, DCV_MONITOR_MAX_GROUPS, n_groups);
    if (!state || reinterpret_cast<uintptr_t>(state) % 8) return fail(DCV_EINVAL, "%s: the state must be non-null and on an 8-byte boundary", who);
    return DCV_OK;
}

}  // namespace dcv

using namespace dcv;

extern "C" {

int dcv_monitor_observe(int n_slots, const float* const* slots, int n_groups, const float* const* groups, const int64_t* group_n, int64_t* state, void* stream) {
    const int rc = mon_check_state("monitor_observe", n_slots, n_groups, state);
    if (rc != DCV_OK) return rc;
    if ((n_slots > 0 && !slots) || (n_groups > 0 && (!groups || !group_n))) return fail(DCV_EINVAL, "monitor_observe: null table");
    MonArgs a;
    memset(&a, 0, sizeof(a));
    a.n_slots = n_slots; a.n_groups = n_groups;
    for (int s = 0; s < n_slots; ++s) {
        if (reinterpret_cast<uintptr_t>(slots[s]) % 4) return fail(DCV_EINVAL, "monitor_observe: slot %d is not on a 4-byte boundary", s);
        a.slot[s] = slots[s];
    }
    for (int g = 0; g < n_groups; ++g) {
        if (!groups[g]) continue;
        if (reinterpret_cast<uintptr_t>(groups[g]) % 4) return fail(DCV_EINVAL, "monitor_observe: group %d is not on a 4-byte boundary", g);
        if (group_n[g] < 1 || group_n[g] > MON_MAX_N) return fail(DCV_EINVAL, "monitor_observe: 1 <= n <= 2^24 logits per group (group %d: %lld)", g, (long long)group_n[g]);
        a.group[g] = groups[g]; a.n[g] = (int32_t)group_n[g];
    }
    hipLaunchKernelGGL(monitor_observe_kernel, dim3((unsigned)n_groups + 1), dim3(256), 0, static_cast<hipStream_t>(stream), a, state);
    DCV_LAUNCH_CHECK();
    return DCV_OK;
}

int dcv_monitor_roll(int n_slots, int n_groups, int64_t* state, int64_t* record, int64_t iteration, void* stream) {
    const int rc = mon_check_state("monitor_roll", n_slots, n_groups, state);
    if (rc != DCV_OK) return rc;
    if (!record || reinterpret_cast<uintptr_t>(record) % 8) return fail(DCV_EINVAL, "monitor_roll: the record must be non-null and on an 8-byte boundary");
    if (record == state) return fail(DCV_EINVAL, "monitor_roll: the record must not be the state");
    hipLaunchKernelGGL(monitor_roll_kernel, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream), n_slots, n_groups, state, record, iteration);
    DCV_LAUNCH_CHECK();
    return DCV_OK;
}

int dcv_hist_u8(const uint8_t* x, int N, int C, int T, int H, int W, int channel, int64_t* counts, int accumulate, void* stream) {
    if (N < 1 || C < 1 || T < 1 || H < 1 || W < 1) return fail(DCV_EINVAL, "hist_u8: every extent of (N, C, T, H, W) must be >= 1 (got %d, %d, %d, %d, %d)", N, C, T, H, W);
    if (channel < 0 || channel >= C) return fail(DCV_EINVAL, "hist_u8: channel %d of %d", channel, C);
    if (!x) return fail(DCV_EINVAL, "hist_u8: null input");
    if (!counts || reinterpret_cast<uintptr_t>(counts) % 8) return fail(DCV_EINVAL, "hist_u8: counts must be 256 int64 on an 8-byte boundary");
    const int64_t run = (int64_t)T * H * W;
    const int64_t chunks = (run + HIST_CHUNK - 1) / HIST_CHUNK;
    if (run > ((int64_t)1 << 40) / C || chunks * N >= ((int64_t)1 << 31)) return fail(DCV_EINVAL, "hist_u8: the tensor is too large (%lld bytes per channel run, %d clips)", (long long)run, N);
    hipStream_t st = static_cast<hipStream_t>(stream);
    unsigned long long* cn = reinterpret_cast<unsigned long long*>(counts);
    if (!accumulate) {
        hipLaunchKernelGGL(hist_zero_kernel, dim3(1), dim3(256), 0, st, cn);
        DCV_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(hist_u8_kernel, dim3((unsigned)(chunks * N)), dim3(256), 0, st, x + (int64_t)channel * run, run, (int64_t)C * run, (int)chunks, cn);
    DCV_LAUNCH_CHECK();
    return DCV_OK;
}

int dcv_video_grid_u8(const uint8_t* geo, const uint8_t* colour, int rows, int cols, int N, int T, int H, int W, uint8_t* out, void* stream) {
    if (rows < 1 || cols < 1 || N < 1 || T < 1 || H < 1 || W < 1) return fail(DCV_EINVAL, "video_grid_u8: rows, cols, N, T, H, W must be >= 1");
    if ((int64_t)rows * cols != N) return fail(DCV_EINVAL, "video_grid_u8: %d clips do not fill a %d x %d grid", N, rows, cols);
    if (!geo || !colour || !out) return fail(DCV_EINVAL, "video_grid_u8: null tensor");
    const int64_t bytes = (int64_t)N * 3 * T * H * W * 2;
    if ((int64_t)N * 3 * T * H > ((int64_t)1 << 38) / W) return fail(DCV_EINVAL, "video_grid_u8: the grid is too large");
    const bool vec = W % 16 == 0 && ((reinterpret_cast<uintptr_t>(geo) | reinterpret_cast<uintptr_t>(colour) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
    const int64_t units = vec ? bytes / 16 : bytes;
    const int64_t blocks = (units + 255) / 256;
    if (blocks >= ((int64_t)1 << 31)) return fail(DCV_EINVAL, "video_grid_u8: the grid is too large");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (vec)
        hipLaunchKernelGGL(video_grid_kernel<uint4>, dim3((unsigned)blocks), dim3(256), 0, st, reinterpret_cast<const uint4*>(geo), reinterpret_cast<const uint4*>(colour),
                           rows, cols, T, H, W / 16, units, reinterpret_cast<uint4*>(out));
    else
        hipLaunchKernelGGL(video_grid_kernel<uint8_t>, dim3((unsigned)blocks), dim3(256), 0, st, geo, colour, rows, cols, T, H, W, units, out);
    DCV_LAUNCH_CHECK();
    return DCV_OK;
}

}  // extern "C"
