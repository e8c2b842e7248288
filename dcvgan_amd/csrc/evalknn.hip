// k-nearest-neighbour manifold metrics on the device, gfx950: improved precision / recall (Kynkaanniemi et al. 2019) and density / coverage (Naeem et al.
// 2020) over features that never leave the device.  The n x n distance matrix is never written: it lives, 64 x 64 at a time, in MFMA accumulators and one LDS tile.
//   eval_row_norms_kernel       norms[i] = sum_d x[i][d]^2                                fp64 VALU, one lane per row, features ascending
//   eval_knn_lists_kernel       per row the k smallest d2 of a share of the columns       the main loop of eval_kid_tiles_kernel without the table; lists in registers
//   eval_knn_merge_kernel       rad2[i] = the k-th smallest over the shares' lists
//   eval_manifold_tiles_kernel  per query: #{support i : d2 <= rad2[i]} and min_i d2     the same main loop; partial counts and minima per share of the columns
//   eval_manifold_fold_kernel   the shares' counts added, their minima folded
//   eval_manifold_reduce_kernel the four integers a metric is a ratio of
// d2(x, y) = max(0, (|x|^2 + |y|^2) - 2 x.y) in fp64, every operation rounded on its own.  Every output element has one owning workgroup; what is combined across
// workgroups (the k smallest of a multiset, integer sums, minima) does not depend on the order, so the results are the same bits for every column split.  No atomic.
#include "dcv_common.h"

namespace dcv {

static const int KN_MAX_D = 4096;      // features per row
static const int KN_TILE = 64;         // a workgroup's tile: 4 waves x (2 x 2) MFMA tiles of 16 x 16
static const int KN_MAX_K = 16;        // neighbours; the length of every list in registers
static const int KN_MAX_SPLITS = 64;   // column shares per row tile
static const int KN_PITCH = 65;        // doubles per row of the LDS distance tile (64 + 1: the four scanning lanes of a row start 16 columns apart)
static const int KN_SLOTS = 32;        // partial results per query row inside a workgroup: 2 waves x 16 lanes

#pragma clang fp contract(off)

// The wave's two 16-row operand blocks starting at row r0: lane l reads row r0 + 16 a + (l & 15).  A row past n is not read (its pointer is row 0's) and counts as zeros.
__device__ __forceinline__ void kn_rows(const float* x, int64_t stride, int n, uint32_t r0, int col, const float* (&p)[2], bool (&live)[2]) {
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        const uint32_t i = r0 + 16 * a + col;      // unsigned: n + 63 may pass 2^31
        live[a] = i < (uint32_t)n;
        p[a] = x + (int64_t)(live[a] ? i : 0) * stride;
    }
}

// acc[a][b] = the 16 x 16 block of dot products of the wave's row block a with its column block b, contraction over the D features: lane l holds features
// d0 + 4 (l >> 4) + q, q = 0 .. 3 of its row — one 16-byte read feeding four MFMAs (VEC: D and the strides multiples of four, the bases on 16-byte boundaries), four
// guarded 4-byte reads otherwise.  eval_kid_tiles_kernel's loop without the table.
template <bool VEC>
__device__ __forceinline__ void kn_tile_dots(const float* const (&pa)[2], const bool (&la)[2], const float* const (&pb)[2], const bool (&lb)[2], int D, int g,
                                             ev_d4 (&acc)[2][2]) {
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = ev_d4{0.0, 0.0, 0.0, 0.0};
    const ev_f4 zero = ev_f4{0.f, 0.f, 0.f, 0.f};
    for (int d0 = 0; d0 < D; d0 += 16) {
        const int d = d0 + 4 * g;
        ev_f4 A[2], B[2];
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            if (VEC) {
                A[a] = (la[a] && d < D) ? *reinterpret_cast<const ev_f4*>(pa[a] + d) : zero;
                B[a] = (lb[a] && d < D) ? *reinterpret_cast<const ev_f4*>(pb[a] + d) : zero;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    A[a][e] = (la[a] && d + e < D) ? pa[a][d + e] : 0.f;
                    B[a][e] = (lb[a] && d + e < D) ? pb[a][d + e] : 0.f;
                }
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b) acc[a][b] = ev_mfma((double)A[a][e], (double)B[b][e], acc[a][b]);
    }
}

__device__ __forceinline__ double kn_d2(double ni, double nj, double dot) {
    const double t = (ni + nj) - 2.0 * dot;
    return t < 0.0 ? 0.0 : t;      // a NaN stays a NaN (fmax would drop it)
}

// An ascending list of KN_MAX_K doubles in registers: v goes in where it belongs and the largest falls out.  Compile-time indices only (a dynamically indexed register
// array lands in scratch); equal values are kept side by side, so the list is the KN_MAX_K smallest of the multiset whatever the order of insertion.
__device__ __forceinline__ void kn_insert(double (&L)[KN_MAX_K], double v) {
#pragma unroll
    for (int i = 0; i < KN_MAX_K; ++i) {
        const bool c = v < L[i];
        const double t = c ? L[i] : v;
        L[i] = c ? v : L[i];
        v = t;
    }
}

// ---- row norms -------------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void eval_row_norms_kernel(const float* __restrict__ x, int n, int D, int64_t stride, double* __restrict__ norms) {
    const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const float* r = x + i * stride;
    double s = 0.0;
    for (int d = 0; d < D; ++d) {
        const double v = (double)r[d];
        s += v * v;
    }
    norms[i] = s;
}

// ---- radii -----------------------------------------------------------------------------------------------------------------------------------------------
// Workgroup (ti, s) owns rows 64 ti .. 64 ti + 63 and sweeps the column tiles s, s + S, ... of the same matrix.  After each tile the accumulators become d2 in the LDS
// tile (+inf for what is dropped: the row itself — by index —, a column past n, a NaN); lane t then scans columns 16 (t & 3) .. + 15 of row t >> 2 into its list; a
// value not below the list's last is rejected at once.  At the end of the sweep the four lists of a row are merged through the same LDS and the row's k smallest go to
// ws[(s n + row) k ..].  No symmetry: an upper tile would have to update the lists of its rows AND of its columns, which ends the rule of one owner per row.
template <bool VEC>
__global__ __launch_bounds__(256) void eval_knn_lists_kernel(const float* __restrict__ x, int64_t stride, int n, int D, const double* __restrict__ norms, int k, int S,
                                                             double* __restrict__ ws) {
    __shared__ double tile[KN_TILE * KN_PITCH];
    const int ti = blockIdx.x, s = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane & 15, g = lane >> 4;
    const int li0 = (wave >> 1) * 32, lj0 = (wave & 1) * 32;
    const int nct = (int)(((int64_t)n + KN_TILE - 1) / KN_TILE);
    const double inf = __builtin_inf();
    const float* pa[2];
    const float* pb[2];
    bool la[2], lb[2];
    kn_rows(x, stride, n, (uint32_t)ti * KN_TILE + li0, col, pa, la);
    double nr[2][4];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const uint32_t gi = (uint32_t)ti * KN_TILE + li0 + 16 * a + g + 4 * r;
            nr[a][r] = gi < (uint32_t)n ? norms[gi] : 0.0;
        }
    double L[KN_MAX_K];
#pragma unroll
    for (int i = 0; i < KN_MAX_K; ++i) L[i] = inf;
    const int srow = threadIdx.x >> 2, part = threadIdx.x & 3;
    for (int tj = s; tj < nct; tj += S) {      // the same trips for every lane of the workgroup
        kn_rows(x, stride, n, (uint32_t)tj * KN_TILE + lj0, col, pb, lb);
        ev_d4 acc[2][2];
        kn_tile_dots<VEC>(pa, la, pb, lb, D, g, acc);
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int lj = lj0 + 16 * b + col;
            const uint32_t gj = (uint32_t)tj * KN_TILE + lj;
            const double nc = gj < (uint32_t)n ? norms[gj] : 0.0;
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int li = li0 + 16 * a + g + 4 * r;
                    const uint32_t gi = (uint32_t)ti * KN_TILE + li;
                    const double d2 = kn_d2(nr[a][r], nc, acc[a][b][r]);
                    const bool keep = gj < (uint32_t)n && gj != gi && d2 == d2;
                    tile[li * KN_PITCH + lj] = keep ? d2 : inf;
                }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const double v = tile[srow * KN_PITCH + 16 * part + j];
            if (v < L[KN_MAX_K - 1]) kn_insert(L, v);
        }
        __syncthreads();      // the tile is free for the next trip
    }
    double* m = tile;         // 256 lists of KN_MAX_K
#pragma unroll
    for (int i = 0; i < KN_MAX_K; ++i) m[threadIdx.x * KN_MAX_K + i] = L[i];
    __syncthreads();
    if (part == 0) {
        for (int p = 1; p < 4; ++p)
#pragma unroll
            for (int i = 0; i < KN_MAX_K; ++i) {
                const double v = m[(threadIdx.x + p) * KN_MAX_K + i];
                if (v < L[KN_MAX_K - 1]) kn_insert(L, v);
            }
        const uint32_t gi = (uint32_t)ti * KN_TILE + srow;
        if (gi < (uint32_t)n) {
            double* o = ws + ((int64_t)s * n + gi) * k;
#pragma unroll
            for (int i = 0; i < KN_MAX_K; ++i)
                if (i < k) o[i] = L[i];
        }
    }
}

// rad2[i] = the k-th smallest of the S lists of row i (+inf where fewer than k distances survived): one lane per row.
__global__ __launch_bounds__(256) void eval_knn_merge_kernel(const double* __restrict__ ws, int n, int k, int S, double* __restrict__ rad2) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double L[KN_MAX_K];
#pragma unroll
    for (int j = 0; j < KN_MAX_K; ++j) L[j] = __builtin_inf();
    for (int s = 0; s < S; ++s) {
        const double* w = ws + ((int64_t)s * n + i) * k;
        for (int j = 0; j < k; ++j) {
            const double v = w[j];
            if (v < L[KN_MAX_K - 1]) kn_insert(L, v);
        }
    }
    double r = L[0];
#pragma unroll
    for (int j = 1; j < KN_MAX_K; ++j) r = j == k - 1 ? L[j] : r;
    rad2[i] = r;
}

// ---- counts and minima -----------------------------------------------------------------------------------------------------------------------------------
// Workgroup (tq, s) owns queries 64 tq .. 64 tq + 63 and sweeps the support tiles s, s + S, ...; a lane keeps, for each of its eight rows, the count of its columns'
// balls the query falls into and the smallest distance (a NaN compares false in both).  At the end the 32 partial results of a row (2 waves x 16 lanes) meet in LDS.
template <bool VEC>
__global__ __launch_bounds__(256) void eval_manifold_tiles_kernel(const float* __restrict__ q, int64_t sq, int nq, const double* __restrict__ qn,
                                                                  const float* __restrict__ x, int64_t sx, int ns, const double* __restrict__ xn,
                                                                  const double* __restrict__ rad2, int D, int S, double* __restrict__ ws_min, int32_t* __restrict__ ws_cnt) {
    __shared__ double smin[KN_TILE * KN_SLOTS];
    __shared__ int32_t scnt[KN_TILE * KN_SLOTS];
    const int tq = blockIdx.x, s = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane & 15, g = lane >> 4;
    const int li0 = (wave >> 1) * 32, lj0 = (wave & 1) * 32;
    const int nct = (int)(((int64_t)ns + KN_TILE - 1) / KN_TILE);
    const double inf = __builtin_inf();
    const float* pa[2];
    const float* pb[2];
    bool la[2], lb[2];
    kn_rows(q, sq, nq, (uint32_t)tq * KN_TILE + li0, col, pa, la);
    double nr[2][4], mn[2][4];
    int32_t cnt[2][4];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const uint32_t gi = (uint32_t)tq * KN_TILE + li0 + 16 * a + g + 4 * r;
            nr[a][r] = gi < (uint32_t)nq ? qn[gi] : 0.0;
            mn[a][r] = inf;
            cnt[a][r] = 0;
        }
    for (int tj = s; tj < nct; tj += S) {
        kn_rows(x, sx, ns, (uint32_t)tj * KN_TILE + lj0, col, pb, lb);
        ev_d4 acc[2][2];
        kn_tile_dots<VEC>(pa, la, pb, lb, D, g, acc);
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const uint32_t gj = (uint32_t)tj * KN_TILE + lj0 + 16 * b + col;
            const bool ok = gj < (uint32_t)ns;
            const double nc = ok ? xn[gj] : 0.0;
            const double rj = (ok && rad2) ? rad2[gj] : -1.0;      // no d2 is <= -1
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double d2 = kn_d2(nr[a][r], nc, acc[a][b][r]);
                    cnt[a][r] += (ok && d2 <= rj) ? 1 : 0;
                    mn[a][r] = (ok && d2 < mn[a][r]) ? d2 : mn[a][r];
                }
        }
    }
    const int slot = (wave & 1) * 16 + col;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int li = li0 + 16 * a + g + 4 * r;
            smin[li * KN_SLOTS + slot] = mn[a][r];
            scnt[li * KN_SLOTS + slot] = cnt[a][r];
        }
    __syncthreads();
    if (threadIdx.x < KN_TILE) {
        const uint32_t gi = (uint32_t)tq * KN_TILE + threadIdx.x;
        double m = inf;
        int32_t c = 0;
        for (int j = 0; j < KN_SLOTS; ++j) {
            const int jj = (j + threadIdx.x) & (KN_SLOTS - 1);      // rotated: the lanes start in different banks
            const double v = smin[threadIdx.x * KN_SLOTS + jj];
            m = v < m ? v : m;
            c += scnt[threadIdx.x * KN_SLOTS + jj];
        }
        if (gi < (uint32_t)nq) {
            ws_min[(int64_t)s * nq + gi] = m;
            ws_cnt[(int64_t)s * nq + gi] = c;
        }
    }
}

__global__ __launch_bounds__(256) void eval_manifold_fold_kernel(const double* __restrict__ ws_min, const int32_t* __restrict__ ws_cnt, int nq, int S,
                                                                 int32_t* __restrict__ count, double* __restrict__ dmin2) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nq) return;
    double m = __builtin_inf();
    int32_t c = 0;
    for (int s = 0; s < S; ++s) {
        const double v = ws_min[(int64_t)s * nq + i];
        m = v < m ? v : m;
        c += ws_cnt[(int64_t)s * nq + i];
    }
    count[i] = c;
    dmin2[i] = m;
}

// out[0] = #{count > 0}, out[1] = sum count, out[2] = #{dmin2 <= own_rad2} (0 without own_rad2), out[3] = #{norms not finite}: one workgroup, lane l takes rows
// l, l + 256, ... into 64-bit integers; their doubles (exact below 2^53) go through the tree.
__global__ __launch_bounds__(256) void eval_manifold_reduce_kernel(const int32_t* __restrict__ count, const double* __restrict__ dmin2, const double* __restrict__ own_rad2,
                                                                   const double* __restrict__ norms, int n, double* __restrict__ out) {
    __shared__ double p[256];
    int64_t a[4] = {0, 0, 0, 0};
    for (int64_t i = threadIdx.x; i < n; i += 256) {
        const int32_t c = count[i];
        a[0] += c > 0 ? 1 : 0;
        a[1] += c;
        if (own_rad2) a[2] += dmin2[i] <= own_rad2[i] ? 1 : 0;
        a[3] += __builtin_fabs(norms[i]) < __builtin_inf() ? 0 : 1;
    }
    for (int j = 0; j < 4; ++j) {
        const double total = ev_tree_sum((double)a[j], p);
        if (threadIdx.x == 0) out[j] = total;
    }
}

static bool kn_misaligned(const void* q, uintptr_t a) { return reinterpret_cast<uintptr_t>(q) % a != 0; }

// The column shares of a sweep: what the caller forces (1 .. 64), or — 0 — as many as keep every workgroup resident at once (two per CU on 256 CUs), at most one
// per column tile.
static int kn_splits(int64_t n_rows, int64_t n_cols, int col_splits) {
    if (col_splits != 0) return col_splits;
    const int64_t nrt = (n_rows + KN_TILE - 1) / KN_TILE, nct = (n_cols + KN_TILE - 1) / KN_TILE;
    int64_t S = 512 / nrt;
    if (S > nct) S = nct;
    if (S > KN_MAX_SPLITS) S = KN_MAX_SPLITS;
    return S < 1 ? 1 : (int)S;
}

static bool kn_vec(int D, const float* a, int64_t sa, const float* b, int64_t sb) {
    return D % 4 == 0 && sa % 4 == 0 && sb % 4 == 0 && !kn_misaligned(a, 16) && !kn_misaligned(b, 16);
}

}  // namespace dcv

using namespace dcv;

extern "C" {

int dcv_eval_row_norms(const float* x, int64_t n, int D, int64_t row_stride, double* norms, void* stream) {
    if (!x || !norms || kn_misaligned(x, 4) || kn_misaligned(norms, 8)) return fail(DCV_EINVAL, "eval_row_norms: null or misaligned pointer");
    if (D < 1 || D > KN_MAX_D) return fail(DCV_EINVAL, "eval_row_norms: 1 <= D <= %d features (got %d)", KN_MAX_D, D);
    if (n < 1 || n > 0x7fffffffll) return fail(DCV_EINVAL, "eval_row_norms: 1 <= n < 2^31 rows (got %lld)", (long long)n);
    if (row_stride < D) return fail(DCV_EINVAL, "eval_row_norms: row_stride %lld is smaller than the row of %d", (long long)row_stride, D);
    hipLaunchKernelGGL(eval_row_norms_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, static_cast<hipStream_t>(stream), x, (int)n, D, row_stride, norms);
    DCV_LAUNCH_CHECK();
    return DCV_OK;
}

size_t dcv_eval_knn_workspace_bytes(int64_t n_rows, int k, int col_splits) {
    if (k < 1 || k > KN_MAX_K || n_rows < (int64_t)k + 1 || n_rows > 0x7fffffffll || col_splits < 0 || col_splits > KN_MAX_SPLITS) return 0;
    return (size_t)kn_splits(n_rows, n_rows, col_splits) * (size_t)n_rows * (size_t)k * sizeof(double);
}

int dcv_eval_knn_radii(const float* x, int64_t n, int D, int64_t row_stride, const double* norms, int k, int col_splits, void* workspace, size_t workspace_bytes,
                       double* rad2, void* stream) {
    if (!x || !norms || !workspace || !rad2 || kn_misaligned(x, 4) || kn_misaligned(norms, 8) || kn_misaligned(workspace, 8) || kn_misaligned(rad2, 8))
        return fail(DCV_EINVAL, "eval_knn_radii: null or misaligned pointer");
    if (D < 1 || D > KN_MAX_D) return fail(DCV_EINVAL, "eval_knn_radii: 1 <= D <= %d features (got %d)", KN_MAX_D, D);
    if (k < 1 || k > KN_MAX_K) return fail(DCV_EINVAL, "eval_knn_radii: 1 <= k <= %d neighbours (got %d)", KN_MAX_K, k);
    if (n < (int64_t)k + 1 || n > 0x7fffffffll) return fail(DCV_EINVAL, "eval_knn_radii: k + 1 <= n < 2^31 rows (got n %lld, k %d)", (long long)n, k);
    if (row_stride < D) return fail(DCV_EINVAL, "eval_knn_radii: row_stride %lld is smaller than the row of %d", (long long)row_stride, D);
    if (col_splits < 0 || col_splits > KN_MAX_SPLITS) return fail(DCV_EINVAL, "eval_knn_radii: 0 <= col_splits <= %d (got %d)", KN_MAX_SPLITS, col_splits);
    const size_t need = dcv_eval_knn_workspace_bytes(n, k, col_splits);
    if (workspace_bytes < need) return fail(DCV_EWORKSPACE, "eval_knn_radii: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    const int S = kn_splits(n, n, col_splits);
    const dim3 grid((unsigned)((n + KN_TILE - 1) / KN_TILE), (unsigned)S);
    hipStream_t st = static_cast<hipStream_t>(stream);
    double* ws = static_cast<double*>(workspace);
    if (kn_vec(D, x, row_stride, x, row_stride)) hipLaunchKernelGGL((eval_knn_lists_kernel<true>), grid, dim3(256), 0, st, x, row_stride, (int)n, D, norms, k, S, ws);
    else hipLaunchKernelGGL((eval_knn_lists_kernel<false>), grid, dim3(256), 0, st, x, row_stride, (int)n, D, norms, k, S, ws);
    DCV_LAUNCH_CHECK();
    hipLaunchKernelGGL(eval_knn_merge_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, ws, (int)n, k, S, rad2);
    DCV_LAUNCH_CHECK();
    return DCV_OK;
}

size_t dcv_eval_manifold_workspace_bytes(int64_t n_queries, int64_t n_support, int col_splits) {
    if (n_queries < 1 || n_queries > 0x7fffffffll || n_support < 1 || n_support > 0x7fffffffll || col_splits < 0 || col_splits > KN_MAX_SPLITS) return 0;
    return (size_t)kn_splits(n_queries, n_support, col_splits) * (size_t)n_queries * (sizeof(double) + sizeof(int32_t));
}

int dcv_eval_manifold_counts(const float* queries, int64_t stride_q, int64_t nq, const double* norms_q, const float* support, int64_t stride_s, int64_t ns,
                             const double* norms_s, const double* rad2, int D, int col_splits, void* workspace, size_t workspace_bytes, int32_t* count, double* dmin2,
                             void* stream) {
    if (!queries || !norms_q || !support || !norms_s || !workspace || !count || !dmin2 || kn_misaligned(queries, 4) || kn_misaligned(support, 4) ||
        kn_misaligned(norms_q, 8) || kn_misaligned(norms_s, 8) || kn_misaligned(rad2, 8) || kn_misaligned(workspace, 8) || kn_misaligned(count, 4) || kn_misaligned(dmin2, 8))
        return fail(DCV_EINVAL, "eval_manifold_counts: null or misaligned pointer");
    if (D < 1 || D > KN_MAX_D) return fail(DCV_EINVAL, "eval_manifold_counts: 1 <= D <= %d features (got %d)", KN_MAX_D, D);
    if (nq < 1 || ns < 1 || nq > 0x7fffffffll || ns > 0x7fffffffll)
        return fail(DCV_EINVAL, "eval_manifold_counts: 1 <= nq, ns < 2^31 (got %lld, %lld)", (long long)nq, (long long)ns);
    if (nq * ns >= (1ll << 53)) return fail(DCV_EINVAL, "eval_manifold_counts: nq * ns must stay below 2^53 (got %lld, %lld)", (long long)nq, (long long)ns);
    if (stride_q < D || stride_s < D)
        return fail(DCV_EINVAL, "eval_manifold_counts: a row stride (%lld, %lld) is smaller than the row of %d", (long long)stride_q, (long long)stride_s, D);
    if (col_splits < 0 || col_splits > KN_MAX_SPLITS) return fail(DCV_EINVAL, "eval_manifold_counts: 0 <= col_splits <= %d (got %d)", KN_MAX_SPLITS, col_splits);
    const size_t need = dcv_eval_manifold_workspace_bytes(nq, ns, col_splits);
    if (workspace_bytes < need) return fail(DCV_EWORKSPACE, "eval_manifold_counts: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    const int S = kn_splits(nq, ns, col_splits);
    const dim3 grid((unsigned)((nq + KN_TILE - 1) / KN_TILE), (unsigned)S);
    hipStream_t st = static_cast<hipStream_t>(stream);
    double* ws_min = static_cast<double*>(workspace);
    int32_t* ws_cnt = reinterpret_cast<int32_t*>(ws_min + (size_t)S * (size_t)nq);
    if (kn_vec(D, queries, stride_q, support, stride_s))
        hipLaunchKernelGGL((eval_manifold_tiles_kernel<true>), grid, dim3(256), 0, st, queries, stride_q, (int)nq, norms_q, support, stride_s, (int)ns, norms_s, rad2, D, S,
                           ws_min, ws_cnt);
    else
        hipLaunchKernelGGL((eval_manifold_tiles_kernel<false>), grid, dim3(256), 0, st, queries, stride_q, (int)nq, norms_q, support, stride_s, (int)ns, norms_s, rad2, D, S,
                           ws_min, ws_cnt);
    DCV_LAUNCH_CHECK();
    hipLaunchKernelGGL(eval_manifold_fold_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, st, ws_min, ws_cnt, (int)nq, S, count, dmin2);
    DCV_LAUNCH_CHECK();
    return DCV_OK;
}

int dcv_eval_manifold_reduce(const int32_t* count, const double* dmin2, const double* own_rad2, const double* norms, int64_t n, double* out, void* stream) {
    if (!count || !dmin2 || !norms || !out || kn_misaligned(count, 4) || kn_misaligned(dmin2, 8) || kn_misaligned(own_rad2, 8) || kn_misaligned(norms, 8) ||
        kn_misaligned(out, 8))
        return fail(DCV_EINVAL, "eval_manifold_reduce: null or misaligned pointer");
    if (n < 1 || n > 0x7fffffffll) return fail(DCV_EINVAL, "eval_manifold_reduce: 1 <= n < 2^31 rows (got %lld)", (long long)n);
    hipLaunchKernelGGL(eval_manifold_reduce_kernel, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream), count, dmin2, own_rad2, norms, (int)n, out);
    DCV_LAUNCH_CHECK();
    return DCV_OK;
}

}  // extern "C"
