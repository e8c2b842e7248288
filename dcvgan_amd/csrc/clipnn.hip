// Nearest-training-clip search on the device-resident dataset, gfx950.  A query clip is T frames of K = H*W*C bytes; a store window (v, s) is T
// consecutive frames of one video of the ClipStore's packed uint8 buffer.  d(q, v, s) = sum over the window's bytes of (q - c)^2, an int64; per query the k windows
// with the smallest (d, v, s) are returned.  Everything is integers: no tolerance anywhere, and the result does not depend on how the work is cut up.
//
//   nn_gemm_kernel     frame-by-frame squared distances of one chunk of store frames: an NT GEMM on v_mfma_i32_32x32x32_i8 over bytes shifted by 128
//                      (x ^ 0x80 = x - 128 as int8; |a'|^2 + |b'|^2 - 2 a'.b' does not depend on the shift), both operands' K contiguous in memory and read
//                      with 16-byte loads straight into the fragments; both squared norms are summed from the same fragments (v_dot4_i32_i8), so the store is read
//                      once and no norm is kept anywhere.  Writes the uint32 tile D[query frame][store frame] of the chunk.
//   nn_window_kernel   clip distances = diagonal sums of D, masked to windows inside one video and outside the excluded one; every workgroup leaves its k best.
//   nn_merge_kernel    the running k best of a query merged with a chunk's candidates, in the fixed order (d, v, s) = (d, first frame of the window).
// No atomics of any kind.  The reference has no counterpart of any of this.
#include "dcv_common.h"

namespace dcv {

typedef int nn_i4 __attribute__((ext_vector_type(4)));
typedef int nn_i16 __attribute__((ext_vector_type(16)));

constexpr int NN_BM = 256;            // query frames per workgroup: 16 clips of 16 frames; a wave owns 64 of them
constexpr int NN_BN = 64;             // store frames per workgroup
constexpr int NN_WB = 1024;           // window starts per workgroup of nn_window_kernel (4 per thread)
constexpr int NN_KMAX = 8;
constexpr int64_t NN_NONE = 0x7fffffffffffffffll;

// (d1, f1) < (d2, f2): windows are ordered by distance, then by their first frame — which, videos lying back to back in index order, is (video, t0) order
__device__ __forceinline__ bool nn_less(int64_t d1, int64_t f1, int64_t d2, int64_t f2) { return d1 < d2 || (d1 == d2 && f1 < f2); }

// the video that owns frame f (0 <= f < starts[N]): the largest v with starts[v] <= f; starts is strictly increasing (every video has a frame)
__device__ __forceinline__ int nn_video_of(const int64_t* __restrict__ starts, int N, int64_t f) {
    int lo = 0, hi = N;      // starts[lo] <= f < starts[hi]
    while (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1);
        if (starts[mid] <= f) lo = mid; else hi = mid;
    }
    return lo;
}

// first frame of table row q's window, or -1 if the row does not name T frames of one video (nothing is read for such a row)
__device__ __forceinline__ int64_t nn_row_first(const int32_t* __restrict__ table, const int64_t* __restrict__ starts, int N, int T, int q) {
    const int32_t v = table[2 * q], t0 = table[2 * q + 1];
    if (v < 0 || v >= N || t0 < 0) return -1;
    const int64_t s = starts[v];
    if ((int64_t)t0 + T > starts[v + 1] - s) return -1;
    return s + t0;
}

// Bytes k .. k + 15 of a frame as four dwords of SHIFTED bytes, all 16 inside the frame.  mask: ~0, or 0 for a frame that does not exist (its pointer is some frame
// that does, so the load needs no branch) — applied AFTER the shift, as a zero byte before it would count as -128.  ALIGNED: every frame starts on a 16-byte
// boundary and K % 16 == 0.
template <bool ALIGNED>
__device__ __forceinline__ nn_i4 nn_frag(const uint8_t* __restrict__ row, int k, uint32_t mask) {
    uint32_t d[4];
    if (ALIGNED) __builtin_memcpy(d, __builtin_assume_aligned(row + k, 16), 16);
    else __builtin_memcpy(d, row + k, 16);
    return nn_i4{(int)((d[0] ^ 0x80808080u) & mask), (int)((d[1] ^ 0x80808080u) & mask), (int)((d[2] ^ 0x80808080u) & mask), (int)((d[3] ^ 0x80808080u) & mask)};
}
// ... in the last K step, where fewer than 16 (or none) of the bytes may lie inside the frame of K bytes: those are read one by one, the others are 0 after the shift
template <bool ALIGNED>
__device__ __forceinline__ nn_i4 nn_frag_tail(const uint8_t* __restrict__ row, int k, int K, uint32_t mask) {
    const int nv = K - k;
    if (nv >= 16) return nn_frag<ALIGNED>(row, k, mask);
    uint32_t d[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < 15; ++j)
        if (j < nv) d[j >> 2] |= (uint32_t)row[k + j] << (8 * (j & 3));
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int vb = nv - 4 * i;      // bytes of this dword inside the frame
        const uint32_t m = vb >= 4 ? 0xffffffffu : vb <= 0 ? 0u : (1u << (8 * vb)) - 1u;
        d[i] = (d[i] ^ 0x80808080u) & m & mask;
    }
    return nn_i4{(int)d[0], (int)d[1], (int)d[2], (int)d[3]};
}

// sum of the squares of the 16 signed bytes
__device__ __forceinline__ int nn_sq(nn_i4 w) {
    int s = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) s = __builtin_amdgcn_sdot4(w[i], w[i], s, false);
    return s;
}

// D[m][c] = sum_j (q_m[j] - frame_{c0 + c}[j])^2 for query frames m < M and chunk columns c < ncols.  Query frame m is frame m of the packed queries, or frame
// m % T of table row m / T's window of the store.  Fragment map of v_mfma_i32_32x32x32_i8: lane l holds row (A) / column (B) l & 31 and 16 of the step's 32 k in
// its four dwords, lane half l >> 5 choosing which 16.  A and B are loaded with the SAME (lane half, byte) -> k assignment, and a dot product does not care in which
// order its k are visited, so the product is right whichever 16 the hardware calls the first; C/D: column = l & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (l >> 5).
// No LDS and no barrier: waves past the last query frame leave at once.
template <bool ALIGNED>
__global__ __launch_bounds__(256) void nn_gemm_kernel(const uint8_t* __restrict__ store, const uint8_t* __restrict__ queries, const int32_t* __restrict__ qtable,
                                                      const int64_t* __restrict__ starts, int N, int T, int M, int K, int64_t c0, int ncols,
                                                      uint32_t* __restrict__ D, int ld) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int m0 = blockIdx.y * NN_BM + wave * 64;
    if (m0 >= M) return;
    const int n0 = blockIdx.x * NN_BN;
    const uint8_t* const some = store + c0 * (int64_t)K;      // a frame that exists: what the lanes of missing rows and columns load (and mask away)
    const uint8_t* arow[2];
    const uint8_t* brow[2];
    uint32_t amask[2], bmask[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int m = m0 + 32 * i + r;
        arow[i] = some;
        amask[i] = 0u;
        if (m < M) {
            if (qtable) {
                const int q = m / T;
                const int64_t f0 = nn_row_first(qtable, starts, N, T, q);
                if (f0 >= 0) { arow[i] = store + (f0 + (m - q * T)) * (int64_t)K; amask[i] = 0xffffffffu; }
            } else {
                arow[i] = queries + (int64_t)m * K;
                amask[i] = 0xffffffffu;
            }
        }
        const int c = n0 + 32 * i + r;
        brow[i] = c < ncols ? store + (c0 + c) * (int64_t)K : some;
        bmask[i] = c < ncols ? 0xffffffffu : 0u;
    }
    nn_i16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0;
    int na[2] = {0, 0}, nb[2] = {0, 0};
    nn_i4 a[2], b[2];
    auto step = [&]() {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            na[i] += nn_sq(a[i]);
            nb[i] += nn_sq(b[i]);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[i], b[j], acc[i][j], 0, 0, 0);
    };
    int kk = 0;
    if (K >= 32) {      // whole K steps: four branch-free loads each, those of step s + 1 in flight while step s multiplies
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            a[i] = nn_frag<ALIGNED>(arow[i], 16 * h, amask[i]);
            b[i] = nn_frag<ALIGNED>(brow[i], 16 * h, bmask[i]);
        }
        for (; kk + 64 <= K; kk += 32) {
            const int k = kk + 32 + 16 * h;
            nn_i4 an[2], bn[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                an[i] = nn_frag<ALIGNED>(arow[i], k, amask[i]);
                bn[i] = nn_frag<ALIGNED>(brow[i], k, bmask[i]);
            }
            step();
#pragma unroll
            for (int i = 0; i < 2; ++i) { a[i] = an[i]; b[i] = bn[i]; }
        }
        step();
        kk += 32;
    }
    if (kk < K) {      // the ragged last step
        const int k = kk + 16 * h;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            a[i] = nn_frag_tail<ALIGNED>(arow[i], k, K, amask[i]);
            b[i] = nn_frag_tail<ALIGNED>(brow[i], k, K, bmask[i]);
        }
        step();
    }
    // the two lane halves hold the two halves of each frame's norm
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        na[i] += __shfl_xor(na[i], 32, 64);
        nb[i] += __shfl_xor(nb[i], 32, 64);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int row = (e & 3) + 8 * (e >> 2) + 4 * h;
            const int qa = __shfl(na[i], row, 64);      // lane `row` loaded query frame m0 + 32 i + row
            const int m = m0 + 32 * i + row;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int c = n0 + 32 * j + r;
                // |a'|^2, |b'|^2 <= 2^30 and |a'.b'| <= 2^30; the distance itself is <= 255^2 * 65536 < 2^32
                if (m < M && c < ncols) D[(int64_t)m * ld + c] = (uint32_t)((int64_t)qa + (int64_t)nb[j] - 2 * (int64_t)acc[i][j][e]);
            }
        }
}

// the block's minimum of (d, f) in the order of nn_less, on every thread; sd / sf: one slot per wave
__device__ __forceinline__ void nn_block_min(int64_t& d, int64_t& f, int64_t* sd, int64_t* sf) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int64_t od = __shfl_xor(d, o, 64), of = __shfl_xor(f, o, 64);
        if (nn_less(od, of, d, f)) { d = od; f = of; }
    }
    __syncthreads();      // the slots' readers of the round before are done
    if ((threadIdx.x & 63) == 0) { sd[threadIdx.x >> 6] = d; sf[threadIdx.x >> 6] = f; }
    __syncthreads();
    d = sd[0]; f = sf[0];
#pragma unroll
    for (int w = 1; w < 4; ++w)
        if (nn_less(sd[w], sf[w], d, f)) { d = sd[w]; f = sf[w]; }
}

// Workgroup (b, q): the window starts c0 + b * 1024 .. + 1023 of query q, four per thread.  A window counts if it starts inside the chunk (w < cf), lies inside ONE
// video (`starts`) and that video is not the query's excluded one.  The k best go to part_d / part_f [q][b][0 .. k), in order; empty places hold (NN_NONE, -1).
// Round i takes the smallest key that is greater than round i - 1's: first frames are distinct, so no flag has to remember what was taken.
__global__ __launch_bounds__(256) void nn_window_kernel(const uint32_t* __restrict__ D, int ld, const int64_t* __restrict__ starts, int N, int T, int64_t F, int64_t c0,
                                                        int cf, const int32_t* __restrict__ qtable, const int32_t* __restrict__ exclude, int exclude_stride, int k,
                                                        int64_t* __restrict__ part_d, int64_t* __restrict__ part_f) {
    __shared__ int64_t sd[4], sf[4];
    const int q = blockIdx.y, b = blockIdx.x;
    const int ex = exclude ? exclude[(int64_t)q * exclude_stride] : -1;
    const bool qok = !qtable || nn_row_first(qtable, starts, N, T, q) >= 0;
    int64_t d[4], f[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int w = b * NN_WB + i * 256 + (int)threadIdx.x;
        f[i] = c0 + w;
        d[i] = NN_NONE;
        if (qok && w < cf && f[i] + T <= F) {
            const int v = nn_video_of(starts, N, f[i]);
            if (f[i] + T <= starts[v + 1] && v != ex) {
                const uint32_t* p = D + (int64_t)q * T * ld + w;
                int64_t s = 0;
                for (int t = 0; t < T; ++t) s += (int64_t)p[(int64_t)t * ld + t];
                d[i] = s;
            }
        }
    }
    int64_t pd = -1, pf = -1;
    for (int i = 0; i < k; ++i) {
        int64_t bd = NN_NONE, bf = NN_NONE;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (d[j] != NN_NONE && nn_less(pd, pf, d[j], f[j]) && nn_less(d[j], f[j], bd, bf)) { bd = d[j]; bf = f[j]; }
        nn_block_min(bd, bf, sd, sf);
        if (threadIdx.x == 0) {
            const int64_t o = ((int64_t)q * gridDim.x + b) * k + i;
            part_d[o] = bd;
            part_f[o] = bd == NN_NONE ? -1 : bf;
        }
        pd = bd; pf = bf;      // once nothing is left, bd = NN_NONE and no key is greater
    }
}

// One workgroup per query: the k best of {the running best (unless first), the chunk's nb * k candidates}, written back as the running best (best_f: first frames,
// dist) and as rows (video, t0).  The old running best is copied to LDS before anything is written.
__global__ __launch_bounds__(256) void nn_merge_kernel(const int64_t* __restrict__ part_d, const int64_t* __restrict__ part_f, int nb, int k, int first,
                                                       int64_t* __restrict__ best_f, int64_t* __restrict__ dist, int32_t* __restrict__ rows,
                                                       const int64_t* __restrict__ starts, int N) {
    __shared__ int64_t sd[4], sf[4], od[NN_KMAX], of[NN_KMAX];
    const int q = blockIdx.x;
    if ((int)threadIdx.x < k) {
        od[threadIdx.x] = first ? NN_NONE : dist[(int64_t)q * k + threadIdx.x];
        of[threadIdx.x] = first ? -1 : best_f[(int64_t)q * k + threadIdx.x];
    }
    __syncthreads();
    const int64_t* qd = part_d + (int64_t)q * nb * k;
    const int64_t* qf = part_f + (int64_t)q * nb * k;
    const int total = nb * k + k;
    int64_t pd = -1, pf = -1;
    for (int i = 0; i < k; ++i) {
        int64_t bd = NN_NONE, bf = NN_NONE;
        for (int c = threadIdx.x; c < total; c += 256) {
            const int64_t cd = c < k ? od[c] : qd[c - k], cfr = c < k ? of[c] : qf[c - k];
            if (cd != NN_NONE && nn_less(pd, pf, cd, cfr) && nn_less(cd, cfr, bd, bf)) { bd = cd; bf = cfr; }
        }
        nn_block_min(bd, bf, sd, sf);
        if (threadIdx.x == 0) {
            const int64_t o = (int64_t)q * k + i;
            dist[o] = bd;
            if (bd == NN_NONE) {
                best_f[o] = -1; rows[2 * o] = -1; rows[2 * o + 1] = -1;
            } else {
                const int v = nn_video_of(starts, N, bf);
                best_f[o] = bf; rows[2 * o] = v; rows[2 * o + 1] = (int32_t)(bf - starts[v]);
            }
        }
        pd = bd; pf = bf;
    }
}

// out[((q T + t) H W + p) C + c] = byte of x[q][c][t][p]: the query frames in the store's disk order.  fp32 values take dcv_videos_to_uint8's arithmetic.
template <class TIN>
__global__ __launch_bounds__(256) void nn_pack_kernel(const TIN* __restrict__ x, dcv_dims5 xd, uint8_t* __restrict__ out, int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    int64_t rest = i;
    const int c = (int)(rest % xd.c); rest /= xd.c;
    const int w = (int)(rest % xd.w); rest /= xd.w;
    const int hh = (int)(rest % xd.h); rest /= xd.h;
    const int t = (int)(rest % xd.d); rest /= xd.d;
    const TIN v = x[rest * xd.sn + c * xd.sc + t * xd.sd + hh * xd.sh + w * xd.sw];
    if constexpr (sizeof(TIN) == 1) {
        out[i] = (uint8_t)v;
    } else {
        float u = fminf(fmaxf((float)v, -1.f), 1.f);
        u = __fmul_rn(__fmul_rn(__fadd_rn(u, 1.f), 0.5f), 255.f);
        out[i] = (uint8_t)(int)u;
    }
}

// out (B, C, T, H, W) = the raw bytes of the table's windows; a row that names no window gives zeros and reads nothing
__global__ __launch_bounds__(256) void nn_gather_u8_kernel(const uint8_t* __restrict__ frames, const int32_t* __restrict__ table, const int64_t* __restrict__ starts,
                                                           int N, int T, int HW, int C, uint8_t* __restrict__ out, int64_t per_clip) {
    const int b = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= per_clip) return;
    const int64_t f0 = nn_row_first(table, starts, N, T, b);
    const int p = (int)(i % HW);
    const int64_t rest = i / HW;
    const int t = (int)(rest % T), c = (int)(rest / T);
    out[(int64_t)b * per_clip + i] = f0 < 0 ? (uint8_t)0 : frames[((f0 + t) * HW + p) * C + c];
}

struct NNLayout {
    size_t best_f, part_d, part_f, D, total;
    int nb, ld;
};
// the workspace of a call whose chunks hold up to chunk_frames window starts each
static NNLayout nn_layout(int n, int T, int k, int64_t chunk_frames) {
    NNLayout L;
    L.nb = (int)((chunk_frames + NN_WB - 1) / NN_WB);
    L.ld = (int)align_up((size_t)(chunk_frames + T - 1), 64);
    size_t o = 0;
    L.best_f = o; o += align_up((size_t)n * k * 8, 256);
    L.part_d = o; o += align_up((size_t)n * L.nb * k * 8, 256);
    L.part_f = o; o += align_up((size_t)n * L.nb * k * 8, 256);
    L.D = o; o += align_up((size_t)n * T * (size_t)L.ld * 4, 256);
    L.total = o;
    return L;
}
static bool nn_sizes_ok(int n, int T, int k, int64_t chunk_frames) {
    return n >= 1 && n <= 65535 && T >= 1 && T <= 4096 && (int64_t)n * T < (1ll << 24) && k >= 1 && k <= NN_KMAX && chunk_frames >= 1 && chunk_frames < (1ll << 30);
}

}  // namespace dcv

using namespace dcv;

extern "C" {

size_t dcv_clipnn_workspace_bytes(int n, int T, int k, int64_t chunk_frames) {
    if (!nn_sizes_ok(n, T, k, chunk_frames)) {
        fail(DCV_EINVAL, "clipnn_workspace_bytes: 1 <= n <= 65535, 1 <= T <= 4096, n T < 2^24, 1 <= k <= 8, 1 <= chunk_frames < 2^30 (got n %d, T %d, k %d, chunk_frames %lld)",
             n, T, k, (long long)chunk_frames);
        return 0;
    }
    return nn_layout(n, T, k, chunk_frames).total;
}

int dcv_clipnn_pack_queries(const void* x, int is_f32, const dcv_dims5* xd, uint8_t* out, void* stream) {
    if (!x || !xd || !out || (is_f32 != 0 && is_f32 != 1)) return fail(DCV_EINVAL, "clipnn_pack_queries: null pointer or is_f32 outside {0, 1}");
    if (is_f32 && reinterpret_cast<uintptr_t>(x) % 4) return fail(DCV_EINVAL, "clipnn_pack_queries: fp32 queries on no 4-byte boundary");
    if (xd->n < 1 || xd->c < 1 || xd->c > 4 || xd->d < 1 || xd->h < 1 || xd->w < 1)
        return fail(DCV_EINVAL, "clipnn_pack_queries: (n, C, T, H, W) with every extent >= 1 and C <= 4 (got %d, %d, %d, %d, %d)", xd->n, xd->c, xd->d, xd->h, xd->w);
    if ((int64_t)xd->h * xd->w * xd->c > 65536) return fail(DCV_EUNSUPPORTED, "clipnn_pack_queries: H*W*C = %lld bytes per frame, at most 65536", (long long)xd->h * xd->w * xd->c);
    const int64_t total = numel(*xd);
    if ((total + 255) / 256 > 0x7fffffffll) return fail(DCV_EINVAL, "clipnn_pack_queries: %lld bytes of queries are too many for one launch", (long long)total);
    const dim3 grid((unsigned)((total + 255) / 256));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (is_f32) hipLaunchKernelGGL((nn_pack_kernel<float>), grid, dim3(256), 0, s, static_cast<const float*>(x), *xd, out, total);
    else hipLaunchKernelGGL((nn_pack_kernel<uint8_t>), grid, dim3(256), 0, s, static_cast<const uint8_t*>(x), *xd, out, total);
    DCV_LAUNCH_CHECK();
    return DCV_OK;
}

int dcv_clipnn_search(const uint8_t* frames, const int64_t* starts, int64_t N, int64_t F, int T, int H, int W, int C, const uint8_t* queries, const int32_t* qtable, int n,
                      const int32_t* exclude, int exclude_stride, int k, int64_t chunk_start, int64_t chunk_frames, int32_t* rows, int64_t* dist, void* ws,
                      size_t ws_bytes, void* stream) {
    if (!frames || !starts || !rows || !dist || !ws) return fail(DCV_EINVAL, "clipnn_search: null pointer");
    if ((queries == nullptr) == (qtable == nullptr)) return fail(DCV_EINVAL, "clipnn_search: exactly one of queries and qtable");
    if (reinterpret_cast<uintptr_t>(starts) % 8 || reinterpret_cast<uintptr_t>(dist) % 8 || reinterpret_cast<uintptr_t>(rows) % 4 || reinterpret_cast<uintptr_t>(ws) % 16 ||
        reinterpret_cast<uintptr_t>(qtable) % 4 || reinterpret_cast<uintptr_t>(exclude) % 4)
        return fail(DCV_EINVAL, "clipnn_search: misaligned pointer (starts, dist: 8 bytes; rows, qtable, exclude: 4; ws: 16)");
    if (H < 1 || W < 1 || C < 1 || C > 4 || N < 1 || N > 0x7fffffffll || F < 1 || F >= (1ll << 31))
        return fail(DCV_EINVAL, "clipnn_search: H, W >= 1, 1 <= C <= 4, 1 <= N < 2^31, 1 <= F < 2^31 (got H %d, W %d, C %d, N %lld, F %lld)", H, W, C, (long long)N, (long long)F);
    const int64_t K64 = (int64_t)H * W * C;
    if (K64 > 65536) return fail(DCV_EUNSUPPORTED, "clipnn_search: H*W*C = %lld bytes per frame, at most 65536 (a frame's dot of shifted bytes must stay below 2^31)", (long long)K64);
    if (!nn_sizes_ok(n, T, k, chunk_frames))
        return fail(DCV_EINVAL, "clipnn_search: 1 <= n <= 65535, 1 <= T <= 4096, n T < 2^24, 1 <= k <= 8, 1 <= chunk_frames < 2^30 (got n %d, T %d, k %d, chunk_frames %lld)", n, T, k,
                    (long long)chunk_frames);
    if (exclude && exclude_stride < 1) return fail(DCV_EINVAL, "clipnn_search: exclude_stride >= 1 (got %d)", exclude_stride);
    const int64_t windows = F - T + 1;      // window starts of the packed buffer, those across a video boundary included (masked in the kernel)
    if (windows < 1 || chunk_start < 0 || chunk_start >= windows || chunk_start % chunk_frames)
        return fail(DCV_EINVAL, "clipnn_search: chunk_start %lld is no multiple of chunk_frames %lld inside the %lld window starts", (long long)chunk_start, (long long)chunk_frames,
                    (long long)windows);
    const NNLayout L = nn_layout(n, T, k, chunk_frames);
    if (ws_bytes < L.total) return fail(DCV_EWORKSPACE, "clipnn_search: %zu bytes of workspace, %zu needed (dcv_clipnn_workspace_bytes)", ws_bytes, L.total);
    const int K = (int)K64, M = n * T;
    const int cf = (int)(windows - chunk_start < chunk_frames ? windows - chunk_start : chunk_frames);
    const int ncols = cf + T - 1;      // chunk_start + ncols <= F
    const int nb = (cf + NN_WB - 1) / NN_WB;
    char* base = static_cast<char*>(ws);
    int64_t* best_f = reinterpret_cast<int64_t*>(base + L.best_f);
    int64_t* part_d = reinterpret_cast<int64_t*>(base + L.part_d);
    int64_t* part_f = reinterpret_cast<int64_t*>(base + L.part_f);
    uint32_t* D = reinterpret_cast<uint32_t*>(base + L.D);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 ggrid((unsigned)((ncols + NN_BN - 1) / NN_BN), (unsigned)((M + NN_BM - 1) / NN_BM));
    const bool aligned = K % 16 == 0 && reinterpret_cast<uintptr_t>(frames) % 16 == 0 && reinterpret_cast<uintptr_t>(queries) % 16 == 0;
    if (aligned) hipLaunchKernelGGL((nn_gemm_kernel<true>), ggrid, dim3(256), 0, s, frames, queries, qtable, starts, (int)N, T, M, K, chunk_start, ncols, D, L.ld);
    else hipLaunchKernelGGL((nn_gemm_kernel<false>), ggrid, dim3(256), 0, s, frames, queries, qtable, starts, (int)N, T, M, K, chunk_start, ncols, D, L.ld);
    DCV_LAUNCH_CHECK();
    hipLaunchKernelGGL(nn_window_kernel, dim3((unsigned)nb, (unsigned)n), dim3(256), 0, s, D, L.ld, starts, (int)N, T, F, chunk_start, cf, qtable, exclude, exclude_stride, k, part_d,
                       part_f);
    DCV_LAUNCH_CHECK();
    hipLaunchKernelGGL(nn_merge_kernel, dim3((unsigned)n), dim3(256), 0, s, part_d, part_f, nb, k, chunk_start == 0 ? 1 : 0, best_f, dist, rows, starts, (int)N);
    DCV_LAUNCH_CHECK();
    return DCV_OK;
}

int dcv_clipnn_gather_u8(const uint8_t* frames, const int32_t* table, const int64_t* starts, int64_t N, int B, int T, int H, int W, int C, uint8_t* out, void* stream) {
    if (!frames || !table || !starts || !out || reinterpret_cast<uintptr_t>(table) % 4 || reinterpret_cast<uintptr_t>(starts) % 8)
        return fail(DCV_EINVAL, "clipnn_gather_u8: null or misaligned pointer");
    if (B < 1 || B > 65535 || T < 1 || H < 1 || W < 1 || C < 1 || C > 4 || N < 1 || N > 0x7fffffffll || (int64_t)H * W >= (1ll << 31))
        return fail(DCV_EINVAL, "clipnn_gather_u8: 1 <= B <= 65535, T, H, W >= 1, 1 <= C <= 4, 1 <= N < 2^31 (got B %d, T %d, H %d, W %d, C %d, N %lld)", B, T, H, W, C, (long long)N);
    const int64_t per_clip = (int64_t)C * T * H * W;
    if ((per_clip + 255) / 256 > 0x7fffffffll) return fail(DCV_EINVAL, "clipnn_gather_u8: a clip of %lld bytes is too large", (long long)per_clip);
    hipLaunchKernelGGL(nn_gather_u8_kernel, dim3((unsigned)((per_clip + 255) / 256), (unsigned)B), dim3(256), 0, static_cast<hipStream_t>(stream), frames, table, starts, (int)N, T,
                       H * W, C, out, per_clip);
    DCV_LAUNCH_CHECK();
    return DCV_OK;
}

}  // extern "C"
