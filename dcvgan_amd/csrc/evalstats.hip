// On-device evaluation statistics, gfx950: what the reference hands to an external package after writing every generated clip to disk
// (trainer.py:171-224) — the accumulations behind the Inception score, the Frechet distance and the kernel distance — over features that never leave the device.
//   eval_moments_kernel      sum += sum_i x_i, gram += X^T X        fp64 matrix pipe (v_mfma_f64_16x16x4_f64), contraction over the rows
//   eval_inception_*         softmax sums of the Inception score    fp64 VALU, per-workgroup partials + a fixed-order fold
//   eval_kid_draw_kernel     the subsets of the kernel distance     the clip store's keyed bijection (dcv_common.h)
//   eval_kid_tiles_kernel    sums of k(x, y) = (x.y / D + 1)^3      the same MFMA, contraction over the feature dimension, rows gathered through the table
// No floating-point atomic anywhere: every output element has one owner and every sum one order, so the same calls give the same bits.
#include "dcv_common.h"

namespace dcv {

static const int EV_MAX_D = 4096;            // features per row, classes per row
static const int EV_TILE = 64;               // a workgroup's output tile: 4 waves x (2 x 2) MFMA tiles of 16 x 16
static const int EV_INCEPTION_GROUPS = 256;  // workgroups (= partial rows in the workspace) of the Inception sums at most
static const int EV_MAX_SUBSETS = 4096;
static const int EV_MAX_SUBSET_SIZE = 65536;

// ev_d4, ev_f4, ev_mfma (v_mfma_f64_16x16x4_f64 and its lane maps) and ev_tree_sum (the order above the lanes) live in dcv_common.h: evalknn.hip shares them.
__device__ __forceinline__ float ev_tree_max(float v, float* p) {      // fmaxf drops a NaN; the NaN itself reaches the sums through exp()
    const int l = threadIdx.x;
    __syncthreads();
    p[l] = v;
    __syncthreads();
#pragma unroll
    for (int s = 128; s >= 1; s >>= 1) {
        if (l < s) p[l] = fmaxf(p[l], p[l + s]);
        __syncthreads();
    }
    return p[0];
}

// ---- feature moments -------------------------------------------------------------------------------------------------------------------------------------
// Workgroup (ti <= tj) owns the 64 x 64 tile (ti, tj) of gram and its mirror image; wave w owns the 32 x 32 quarter (w >> 1, w & 1) as 2 x 2 MFMA tiles whose
// accumulators START from the stored values, then take the rows in ascending order, four per instruction.  With the contraction over the rows the A operand of
// output rows i0 .. i0 + 15 is X[r0 + (l >> 4)][i0 + (l & 15)] and the B operand of columns j0 .. is the same expression with j0: 16 consecutive floats of four
// consecutive rows, straight from memory.  A row past n or a column past D is loaded as zero (a padded row is zero in BOTH operands, a padded column only feeds
// accumulators that are never stored: a NaN elsewhere cannot leak through 0 * NaN).  Tile (i, j) and tile (j, i) of a diagonal workgroup form the same products in the
// same order, so the stored matrix is symmetric bit for bit.  The diagonal workgroups also own sum[]: lane t of wave 0 adds column ti * 64 + t, rows ascending.
__global__ __launch_bounds__(256) void eval_moments_kernel(const float* __restrict__ x, int n, int D, int64_t stride, double* __restrict__ sum, double* __restrict__ gram) {
    const int ti = blockIdx.y, tj = blockIdx.x;
    if (tj < ti) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane & 15, g = lane >> 4;
    const int i0 = ti * EV_TILE + (wave >> 1) * 32, j0 = tj * EV_TILE + (wave & 1) * 32;
    ev_d4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = i0 + 16 * a + g + 4 * r, c = j0 + 16 * b + col;
                acc[a][b][r] = (row < D && c < D) ? gram[(int64_t)row * D + c] : 0.0;
            }
    const int ca[2] = {i0 + col, i0 + 16 + col}, cb[2] = {j0 + col, j0 + 16 + col};
    const bool va[2] = {ca[0] < D, ca[1] < D}, vb[2] = {cb[0] < D, cb[1] < D};
    for (int64_t r0 = 0; r0 < n; r0 += 16) {      // four instructions' rows per trip, all loads first; the rows past n are zeros, and acc + 0 * 0 is acc
        double A[4][2], B[4][2];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t row = r0 + 4 * u + g;
            const bool rv = row < n;
            const float* xr = x + (rv ? row : 0) * stride;
#pragma unroll
            for (int a = 0; a < 2; ++a) A[u][a] = (rv && va[a]) ? (double)xr[ca[a]] : 0.0;
#pragma unroll
            for (int b = 0; b < 2; ++b) B[u][b] = (rv && vb[b]) ? (double)xr[cb[b]] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b) acc[a][b] = ev_mfma(A[u][a], B[u][b], acc[a][b]);
    }
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = i0 + 16 * a + g + 4 * r, c = j0 + 16 * b + col;
                if (row < D && c < D) {
                    gram[(int64_t)row * D + c] = acc[a][b][r];
                    if (ti != tj) gram[(int64_t)c * D + row] = acc[a][b][r];
                }
            }
    if (ti == tj && threadIdx.x < EV_TILE) {
        const int c = ti * EV_TILE + threadIdx.x;
        if (c < D) {
            double s = sum[c];
            for (int64_t r = 0; r < n; ++r) s += (double)x[r * stride + c];
            sum[c] = s;
        }
    }
}

// ---- Inception-score sums --------------------------------------------------------------------------------------------------------------------------------
// Every operation below is rounded on its own (the numpy restatement of tests/test_evaluation_gpu.py follows it line by line).
#pragma clang fp contract(off)

// Workgroup g of G takes rows g, g + G, ...; lane t holds classes t, t + 256, ... (K <= 4096: 16 per lane).  Per row, in double: m = the row maximum,
// e_k = exp(z_k - m), S = sum e_k (lane order, then the tree), p_k = e_k / S, log p_k = (z_k - m) - log S.  The lane keeps sum_i p_ik per class and one running
// sum of p log p (a class with p = 0 adds nothing); the workgroup leaves K + 1 partial sums in its row of the workspace.
__global__ __launch_bounds__(256) void eval_inception_rows_kernel(const float* __restrict__ logits, int n, int K, int64_t stride, int G, double* __restrict__ ws) {
    __shared__ double p[256];
    __shared__ float pm[256];
    const int t = threadIdx.x, g = blockIdx.x;
    double acc[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] = 0.0;
    double ent = 0.0;
    for (int64_t i = g; i < n; i += G) {
        const float* z = logits + i * stride;
        float zf[16];
        float mx = -__builtin_inff();
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int k = t + 256 * j;
            zf[j] = k < K ? z[k] : -__builtin_inff();
            mx = fmaxf(mx, zf[j]);
        }
        const double m = (double)ev_tree_max(mx, pm);
        double e[16], s = 0.0;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int k = t + 256 * j;
            if (k < K) {
                e[j] = exp((double)zf[j] - m);
                s += e[j];
            } else {
                e[j] = 0.0;
            }
        }
        const double S = ev_tree_sum(s, p);
        const double logS = log(S);
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int k = t + 256 * j;
            if (k < K) {
                const double pk = e[j] / S;
                const double lp = ((double)zf[j] - m) - logS;
                acc[j] += pk;
                const double term = pk * lp;
                ent += pk == 0.0 ? 0.0 : term;
            }
        }
    }
    double* o = ws + (int64_t)g * (K + 1);
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int k = t + 256 * j;
        if (k < K) o[k] = acc[j];
    }
    const double E = ev_tree_sum(ent, p);
    if (t == 0) o[K] = E;
}

// state[k] += (((ws[0][k] + ws[1][k]) + ws[2][k]) + ...): one thread per entry, the workgroups' partials in ascending order.
__global__ __launch_bounds__(256) void eval_inception_fold_kernel(const double* __restrict__ ws, int G, int K, double* __restrict__ state) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k > K) return;
    double s = 0.0;
    for (int g = 0; g < G; ++g) s += ws[(int64_t)g * (K + 1) + k];
    state[k] = state[k] + s;
}

// ---- kernel distance -------------------------------------------------------------------------------------------------------------------------------------
// table[s][side][i] = perm_{seed, s, side}(i), i < m: the first m images of a keyed permutation of [0, na) (side 0) or [0, nb) (side 1); clip_perm with the subset in
// the counter's epoch-low word and the side in its epoch-high word.
__global__ __launch_bounds__(256) void eval_kid_draw_kernel(int32_t* __restrict__ table, int64_t total, int m, uint32_t na, uint32_t nb, int ha, int hb, uint32_t k0,
                                                            uint32_t k1) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const uint32_t i = (uint32_t)(idx % m);
    const int64_t rest = idx / m;
    const uint32_t side = (uint32_t)(rest & 1), s = (uint32_t)(rest >> 1);
    table[idx] = (int32_t)clip_perm(i, side ? nb : na, side ? hb : ha, k0, k1, s, side);
}

// Tiles of one subset, in the order of its partials: the nt (nt + 1) / 2 upper tiles (ti <= tj, row by row) of the a-a block, the same of the b-b block, then the
// nt^2 tiles of the a-b block.  An off-diagonal tile of a symmetric block stands for its mirror image too: its partial is doubled (exactly).
// The contraction runs over the features: the A operand of subset rows i0 .. i0 + 15 is row table[i0 + (l & 15)] at features d0 + 4 (l >> 4) + q, q = 0 .. 3 — one
// 16-byte read per lane feeds four MFMAs (VEC: D and the strides multiples of four, the bases on 16-byte boundaries; else four guarded 4-byte reads) — and the B
// operand is the same expression over the column side's rows.  The m x m matrix lives in the accumulators only: the epilogue forms t = dot / D + 1, t * t * t,
// drops what lies outside the subset and the diagonal of a symmetric block, and reduces the tile (lane: its 16 values in (a, b, r) order; then the tree).
// A table entry outside [0, rows) is not followed: its row counts as NaN.
template <bool VEC>
__global__ __launch_bounds__(256) void eval_kid_tiles_kernel(const float* __restrict__ fa, int64_t sa, int na, const float* __restrict__ fb, int64_t sb, int nb, int D,
                                                             const int32_t* __restrict__ table, int m, int nt, int tri, double* __restrict__ ws) {
    __shared__ double p[256];
    const int s = blockIdx.y;
    const int P = 2 * tri + nt * nt;
    int q = blockIdx.x, blk, ti, tj;
    if (q < 2 * tri) {
        blk = q >= tri ? 1 : 0;
        if (blk) q -= tri;
        ti = 0;
        while (q >= nt - ti) { q -= nt - ti; ++ti; }
        tj = ti + q;
    } else {
        blk = 2;
        q -= 2 * tri;
        ti = q / nt; tj = q % nt;
    }
    const bool rows_b = blk == 1, cols_b = blk != 0;
    const float* fr = rows_b ? fb : fa;
    const float* fc = cols_b ? fb : fa;
    const int64_t sr = rows_b ? sb : sa, sc = cols_b ? sb : sa;
    const int nr = rows_b ? nb : na, nc = cols_b ? nb : na;
    const int32_t* tr = table + ((int64_t)s * 2 + (rows_b ? 1 : 0)) * m;
    const int32_t* tc = table + ((int64_t)s * 2 + (cols_b ? 1 : 0)) * m;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane & 15, g = lane >> 4;
    const int i0 = ti * EV_TILE + (wave >> 1) * 32, j0 = tj * EV_TILE + (wave & 1) * 32;
    const float* pa[2];
    const float* pb[2];
    bool la[2], lb[2], na_[2], nb_[2];      // live (inside the subset); named by the table but outside the feature matrix
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        const int i = i0 + 16 * a + col;
        la[a] = i < m;
        const int32_t idx = la[a] ? tr[i] : 0;
        const bool ok = (uint32_t)idx < (uint32_t)nr;
        na_[a] = la[a] && !ok;
        pa[a] = fr + (int64_t)(ok ? idx : 0) * sr;
        const int j = j0 + 16 * a + col;
        lb[a] = j < m;
        const int32_t jdx = lb[a] ? tc[j] : 0;
        const bool okb = (uint32_t)jdx < (uint32_t)nc;
        nb_[a] = lb[a] && !okb;
        pb[a] = fc + (int64_t)(okb ? jdx : 0) * sc;
    }
    ev_d4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = ev_d4{0.0, 0.0, 0.0, 0.0};
    const float nanf_ = __builtin_nanf("");
    for (int d0 = 0; d0 < D; d0 += 16) {
        const int d = d0 + 4 * g;
        ev_f4 A[2], B[2];
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            if (VEC) {
                A[a] = d < D ? *reinterpret_cast<const ev_f4*>(pa[a] + d) : ev_f4{0.f, 0.f, 0.f, 0.f};
                B[a] = d < D ? *reinterpret_cast<const ev_f4*>(pb[a] + d) : ev_f4{0.f, 0.f, 0.f, 0.f};
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    A[a][e] = d + e < D ? pa[a][d + e] : 0.f;
                    B[a][e] = d + e < D ? pb[a][d + e] : 0.f;
                }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                A[a][e] = la[a] ? (na_[a] ? nanf_ : A[a][e]) : 0.f;
                B[a][e] = lb[a] ? (nb_[a] ? nanf_ : B[a][e]) : 0.f;
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b) acc[a][b] = ev_mfma((double)A[a][e], (double)B[b][e], acc[a][b]);
    }
    const double dD = (double)D;
    double v = 0.0;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int gi = i0 + 16 * a + g + 4 * r, gj = j0 + 16 * b + col;
                const double t = acc[a][b][r] / dD + 1.0;
                const double t2 = t * t;
                const double k3 = t2 * t;
                const bool keep = gi < m && gj < m && !(blk < 2 && gi == gj);
                v += keep ? k3 : 0.0;
            }
    double total = ev_tree_sum(v, p);
    if (blk < 2 && ti != tj) total = total + total;
    if (threadIdx.x == 0) ws[(int64_t)s * P + blockIdx.x] = total;
}

// out[3 s + c] = the sum of subset s's partials of block c: lane l adds partials l, l + 256, ... in increasing index, then the tree.
__global__ __launch_bounds__(256) void eval_kid_fold_kernel(const double* __restrict__ ws, int nt, int tri, double* __restrict__ out) {
    __shared__ double p[256];
    const int s = blockIdx.x;
    const int P = 2 * tri + nt * nt;
    const double* w = ws + (int64_t)s * P;
    const int lo[3] = {0, tri, 2 * tri}, hi[3] = {tri, 2 * tri, P};
    for (int c = 0; c < 3; ++c) {
        double v = 0.0;
        for (int i = lo[c] + (int)threadIdx.x; i < hi[c]; i += 256) v += w[i];
        const double total = ev_tree_sum(v, p);
        if (threadIdx.x == 0) out[3 * s + c] = total;
    }
}

static bool misaligned(const void* q, uintptr_t a) { return reinterpret_cast<uintptr_t>(q) % a != 0; }

static bool kid_shape(int subsets, int m, int* nt, int* tri, int64_t* partials) {
    if (subsets < 1 || subsets > EV_MAX_SUBSETS || m < 2 || m > EV_MAX_SUBSET_SIZE) return false;
    *nt = (m + EV_TILE - 1) / EV_TILE;
    *tri = *nt * (*nt + 1) / 2;
    *partials = (int64_t)subsets * (2 * (int64_t)*tri + (int64_t)*nt * *nt);
    return true;
}

}  // namespace dcv

using namespace dcv;

extern "C" {

int dcv_eval_moments_update(const float* x, int64_t n, int D, int64_t row_stride, double* sum, double* gram, void* stream) {
    if (!x || !sum || !gram || misaligned(x, 4) || misaligned(sum, 8) || misaligned(gram, 8)) return fail(DCV_EINVAL, "eval_moments_update: null or misaligned pointer");
    if (D < 1 || D > EV_MAX_D) return fail(DCV_EINVAL, "eval_moments_update: 1 <= D <= %d features (got %d)", EV_MAX_D, D);
    if (n < 1 || n > 0x7fffffffll) return fail(DCV_EINVAL, "eval_moments_update: 1 <= n < 2^31 rows (got %lld)", (long long)n);
    if (row_stride < D) return fail(DCV_EINVAL, "eval_moments_update: row_stride %lld is smaller than the row of %d", (long long)row_stride, D);
    const unsigned nt = (unsigned)((D + EV_TILE - 1) / EV_TILE);
    hipLaunchKernelGGL(eval_moments_kernel, dim3(nt, nt), dim3(256), 0, static_cast<hipStream_t>(stream), x, (int)n, D, row_stride, sum, gram);
    DCV_LAUNCH_CHECK();
    return DCV_OK;
}

size_t dcv_eval_inception_workspace_bytes(int64_t n, int K) {
    if (n < 1 || n > 0x7fffffffll || K < 1 || K > EV_MAX_D) return 0;
    const int64_t G = n < EV_INCEPTION_GROUPS ? n : EV_INCEPTION_GROUPS;
    return (size_t)G * (size_t)(K + 1) * sizeof(double);
}

int dcv_eval_inception_update(const float* logits, int64_t n, int K, int64_t row_stride, double* state, void* workspace, size_t workspace_bytes, void* stream) {
    if (!logits || !state || !workspace || misaligned(logits, 4) || misaligned(state, 8) || misaligned(workspace, 8))
        return fail(DCV_EINVAL, "eval_inception_update: null or misaligned pointer");
    if (K < 1 || K > EV_MAX_D) return fail(DCV_EINVAL, "eval_inception_update: 1 <= K <= %d classes (got %d)", EV_MAX_D, K);
    if (n < 1 || n > 0x7fffffffll) return fail(DCV_EINVAL, "eval_inception_update: 1 <= n < 2^31 rows (got %lld)", (long long)n);
    if (row_stride < K) return fail(DCV_EINVAL, "eval_inception_update: row_stride %lld is smaller than the row of %d", (long long)row_stride, K);
    const size_t need = dcv_eval_inception_workspace_bytes(n, K);
    if (workspace_bytes < need) return fail(DCV_EWORKSPACE, "eval_inception_update: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    const int G = (int)(n < EV_INCEPTION_GROUPS ? n : EV_INCEPTION_GROUPS);
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(eval_inception_rows_kernel, dim3((unsigned)G), dim3(256), 0, s, logits, (int)n, K, row_stride, G, static_cast<double*>(workspace));
    DCV_LAUNCH_CHECK();
    hipLaunchKernelGGL(eval_inception_fold_kernel, dim3((unsigned)((K + 1 + 255) / 256)), dim3(256), 0, s, static_cast<const double*>(workspace), G, K, state);
    DCV_LAUNCH_CHECK();
    return DCV_OK;
}

int dcv_eval_kid_draw(int32_t* table, int subsets, int m, int64_t na, int64_t nb, uint64_t seed, void* stream) {
    if (!table || misaligned(table, 4)) return fail(DCV_EINVAL, "eval_kid_draw: null or misaligned table");
    if (subsets < 1 || subsets > EV_MAX_SUBSETS || m < 2 || m > EV_MAX_SUBSET_SIZE)
        return fail(DCV_EINVAL, "eval_kid_draw: 1 <= subsets <= %d, 2 <= m <= %d (got %d, %d)", EV_MAX_SUBSETS, EV_MAX_SUBSET_SIZE, subsets, m);
    if (na < m || nb < m || na > 0x7fffffffll || nb > 0x7fffffffll)
        return fail(DCV_EINVAL, "eval_kid_draw: m <= na, nb < 2^31 (got m %d, na %lld, nb %lld)", m, (long long)na, (long long)nb);
    const uint64_t key = seed + DCV_EVAL_KID_SALT;
    const int64_t total = (int64_t)subsets * 2 * m;
    hipLaunchKernelGGL(eval_kid_draw_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), table, total, m, (uint32_t)na,
                       (uint32_t)nb, clip_perm_half_bits(na), clip_perm_half_bits(nb), (uint32_t)key, (uint32_t)(key >> 32));
    DCV_LAUNCH_CHECK();
    return DCV_OK;
}

size_t dcv_eval_kid_workspace_bytes(int subsets, int m) {
    int nt, tri;
    int64_t partials;
    if (!kid_shape(subsets, m, &nt, &tri, &partials)) return 0;
    return (size_t)partials * sizeof(double);
}

int dcv_eval_kid_sums(const float* fa, int64_t stride_a, int64_t na, const float* fb, int64_t stride_b, int64_t nb, int D, const int32_t* table, int subsets, int m,
                      void* workspace, size_t workspace_bytes, double* out, void* stream) {
    if (!fa || !fb || !table || !workspace || !out || misaligned(fa, 4) || misaligned(fb, 4) || misaligned(table, 4) || misaligned(workspace, 8) || misaligned(out, 8))
        return fail(DCV_EINVAL, "eval_kid_sums: null or misaligned pointer");
    int nt, tri;
    int64_t partials;
    if (!kid_shape(subsets, m, &nt, &tri, &partials))
        return fail(DCV_EINVAL, "eval_kid_sums: 1 <= subsets <= %d, 2 <= m <= %d (got %d, %d)", EV_MAX_SUBSETS, EV_MAX_SUBSET_SIZE, subsets, m);
    if (D < 1 || D > EV_MAX_D) return fail(DCV_EINVAL, "eval_kid_sums: 1 <= D <= %d features (got %d)", EV_MAX_D, D);
    if (na < 1 || nb < 1 || na > 0x7fffffffll || nb > 0x7fffffffll) return fail(DCV_EINVAL, "eval_kid_sums: 1 <= na, nb < 2^31 (got %lld, %lld)", (long long)na, (long long)nb);
    if (stride_a < D || stride_b < D)
        return fail(DCV_EINVAL, "eval_kid_sums: a row stride (%lld, %lld) is smaller than the row of %d", (long long)stride_a, (long long)stride_b, D);
    if (workspace_bytes < (size_t)partials * sizeof(double))
        return fail(DCV_EWORKSPACE, "eval_kid_sums: workspace of %zu bytes, %zu needed", workspace_bytes, (size_t)partials * sizeof(double));
    const dim3 grid((unsigned)(2 * tri + nt * nt), (unsigned)subsets);
    hipStream_t s = static_cast<hipStream_t>(stream);
    double* ws = static_cast<double*>(workspace);
    const bool vec = D % 4 == 0 && stride_a % 4 == 0 && stride_b % 4 == 0 && !misaligned(fa, 16) && !misaligned(fb, 16);
    if (vec) hipLaunchKernelGGL((eval_kid_tiles_kernel<true>), grid, dim3(256), 0, s, fa, stride_a, (int)na, fb, stride_b, (int)nb, D, table, m, nt, tri, ws);
    else hipLaunchKernelGGL((eval_kid_tiles_kernel<false>), grid, dim3(256), 0, s, fa, stride_a, (int)na, fb, stride_b, (int)nb, D, table, m, nt, tri, ws);
    DCV_LAUNCH_CHECK();
    hipLaunchKernelGGL(eval_kid_fold_kernel, dim3((unsigned)subsets), dim3(256), 0, s, ws, nt, tri, out);
    DCV_LAUNCH_CHECK();
    return DCV_OK;
}

}  // extern "C"
