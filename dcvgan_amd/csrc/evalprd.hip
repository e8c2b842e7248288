// PRD on the device, gfx950: the k-means behind "Assessing Generative Models via Precision and Recall" (Sajjadi et al. 2018; the reference's third metric,
// trainer.py:216-219) over features that never leave the device.  The union of the real rows (A, na) and the fake rows (B, nb) is never copied together: row u of
// the union is a_u for u < na, else b_{u - na}.  R independent runs of C clusters each, full-batch Lloyd; the centroids are one (R, C, D) fp64 tensor.
//   eval_prd_seed_kernel      cent[r][c] = union row perm_r(c)                          the clip store's keyed bijection (dcv_common.h)
//   eval_prd_cn_kernel        cn[r][c] = sum_d cent[r][c][d]^2                          fp64 VALU, features ascending
//   eval_prd_assign_kernel    assign[r][u] = the lowest c of minimal cn - 2 x_u.cent    fp64 matrix pipe, contraction over D; 1, 2 or 4 runs per 64-column tile
//   eval_prd_count_kernel     hist[r][side][c] = rows assigned (column C: unassigned)   integers
//   eval_prd_sums_kernel      partial[s][r][c][d] = sum of x_u[d] over slab s           fp64 matrix pipe, contraction over the rows, A = the selector assign == c
//   eval_prd_fold_kernel      cent = (slabs ascending) / count, where count > 0
// No floating-point atomic: every output element has one owner and every sum one order, so the same calls give the same bits.
#include "dcv_common.h"

namespace dcv {

static const int PRD_MAX_D = 4096;       // features per row
static const int PRD_TILE = 64;          // a workgroup's tile: 4 waves x (2 x 2) MFMA tiles of 16 x 16
static const int PRD_MAX_C = 64;         // clusters per run: one column tile
static const int PRD_MAX_R = 64;         // runs
static const int PRD_MAX_SPLITS = 64;    // row slabs of the update
static const int PRD_PITCH = 65;         // doubles per row of the LDS score tile, as in evalknn.hip

typedef double prd_d2 __attribute__((ext_vector_type(2)));

#pragma clang fp contract(off)

struct PrdUnion {      // the two sides of the union
    const float* fa;
    const float* fb;
    int64_t sa, sb;
    uint32_t na, n;
};

__device__ __forceinline__ const float* prd_row(const PrdUnion& U, uint32_t u) { return u < U.na ? U.fa + (int64_t)u * U.sa : U.fb + (int64_t)(u - U.na) * U.sb; }

__device__ __forceinline__ bool prd_finite(double v) { return __builtin_fabs(v) < __builtin_inf(); }

// ---- seeding ---------------------------------------------------------------------------------------------------------------------------------------------
// Workgroup q = r C + c gathers union row clip_perm(c) of run r — the run in the counter's word where the kernel distance's draw puts the subset — as doubles.
__global__ __launch_bounds__(256) void eval_prd_seed_kernel(PrdUnion U, int D, int C, int h, uint32_t k0, uint32_t k1, double* __restrict__ cent) {
    const int q = blockIdx.x;
    const uint32_t r = (uint32_t)(q / C), c = (uint32_t)(q % C);
    const uint32_t u = clip_perm(c, U.n, h, k0, k1, r, 0u);
    const float* x = prd_row(U, u);
    for (int d = threadIdx.x; d < D; d += 256) cent[(int64_t)q * D + d] = (double)x[d];
}

// ---- assignment ------------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void eval_prd_cn_kernel(const double* __restrict__ cent, int Q, int D, double* __restrict__ cn) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= Q) return;
    const double* c = cent + (int64_t)q * D;
    double s = 0.0;
    for (int d = 0; d < D; ++d) {
        const double v = c[d];
        s += v * v;
    }
    cn[q] = s;
}

// kn_tile_dots (evalknn.hip) with fp64 columns: acc[a][b] = the 16 x 16 block of dot products of the wave's union rows (block a, fp32 converted on load) with its
// centroids (block b, fp64 as they are), contraction over D in the same order: lane l holds features d0 + 4 (l >> 4) + e, e = 0 .. 3, of its row and of its centroid —
// one 16-byte read and two 16-byte reads feeding four MFMAs (VEC), guarded single reads otherwise.  Column block b is formed only for b < nb (wave-uniform): the
// dead blocks (past a run's C clusters, past the last run) are never read and stay zero; a dead block 0 has a dead block 1.
template <bool VEC>
__device__ __forceinline__ void prd_tile_dots(const float* const (&pa)[2], const bool (&la)[2], const double* const (&pb)[2], const bool (&lb)[2], int D, int g, int nb,
                                              ev_d4 (&acc)[2][2]) {
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = ev_d4{0.0, 0.0, 0.0, 0.0};
    if (nb <= 0) return;
    const ev_f4 zero = ev_f4{0.f, 0.f, 0.f, 0.f};
    const prd_d2 zero2 = prd_d2{0.0, 0.0};
    for (int d0 = 0; d0 < D; d0 += 16) {
        const int d = d0 + 4 * g;
        ev_f4 A[2];
        double B[2][4];
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            if (VEC) {
                A[a] = (la[a] && d < D) ? *reinterpret_cast<const ev_f4*>(pa[a] + d) : zero;
                const bool lv = lb[a] && d < D;
                const prd_d2 lo = lv ? *reinterpret_cast<const prd_d2*>(pb[a] + d) : zero2;
                const prd_d2 hi = lv ? *reinterpret_cast<const prd_d2*>(pb[a] + d + 2) : zero2;
                B[a][0] = lo[0]; B[a][1] = lo[1]; B[a][2] = hi[0]; B[a][3] = hi[1];
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    A[a][e] = (la[a] && d + e < D) ? pa[a][d + e] : 0.f;
                    B[a][e] = (lb[a] && d + e < D) ? pb[a][d + e] : 0.0;
                }
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                acc[a][0] = ev_mfma((double)A[a][e], B[0][e], acc[a][0]);
                if (nb > 1) acc[a][1] = ev_mfma((double)A[a][e], B[1][e], acc[a][1]);
            }
    }
}

// Workgroup (ti, s) owns union rows 64 ti .. 64 ti + 63 and takes the column tiles s, s + RS, ...: the row tile stays in the caches for all of them.  A column tile
// holds 64 / W runs, W = 16, 32 or 64 columns each (the smallest that holds the C clusters: two runs per tile at the default 20), run r's clusters in the first C
// columns of its segment; a 16-column block past C or past the last run is never read.  After each tile the scores cn - 2 dot go to the LDS tile (NaN for a dead
// column); lane t scans columns 16 (t & 3) .. + 15 of row t >> 2 in ascending order with a strict <, the parts of a run's segment are merged in ascending order
// with the same rule: the lowest column of the minimal score among those that are not NaN — the minimum of the pairs (score, column), whatever the order of
// merging.  A score's arithmetic does not depend on where its column lies in the tile.
template <bool VEC>
__global__ __launch_bounds__(256) void eval_prd_assign_kernel(PrdUnion U, const double* __restrict__ norms_a, const double* __restrict__ norms_b, int D,
                                                              const double* __restrict__ cent, const double* __restrict__ cn, int C, int R, int W, int RS,
                                                              int32_t* __restrict__ assign) {
    __shared__ double tile[PRD_TILE * PRD_PITCH];
    __shared__ double sbest[256];
    __shared__ int32_t sidx[256];
    const int ti = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane & 15, g = lane >> 4;
    const int li0 = (wave >> 1) * 32, lj0 = (wave & 1) * 32;
    const int P = PRD_TILE / W;                      // runs per column tile
    const int G = (R + P - 1) / P;                   // column tiles
    const double qnan = __builtin_nan("");
    const float* pa[2];
    bool la[2];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        const uint32_t u = (uint32_t)ti * PRD_TILE + li0 + 16 * a + col;      // unsigned: n + 63 may pass 2^31
        la[a] = u < U.n;
        pa[a] = prd_row(U, la[a] ? u : 0u);
    }
    const int srow = threadIdx.x >> 2, part = threadIdx.x & 3;
    const int pseg = (16 * part) / W, pc0 = (16 * part) % W;      // the run segment of this lane's 16 scanned columns, and their first cluster
    const uint32_t gu = (uint32_t)ti * PRD_TILE + srow;
    bool row_ok = false;
    if (gu < U.n) row_ok = prd_finite(gu < U.na ? norms_a[gu] : norms_b[gu - U.na]);
    for (int tj = blockIdx.y; tj < G; tj += RS) {      // the same trips for every lane of the workgroup
        const double* pb[2];
        bool lb[2];
        int rq[2];
        int nb = 0;
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int lj = lj0 + 16 * b + col;
            const int r = tj * P + lj / W, c = lj % W;
            lb[b] = c < C && r < R;
            rq[b] = lb[b] ? r * C + c : 0;
            pb[b] = cent + (int64_t)rq[b] * D;
            const int c0 = (lj0 + 16 * b) % W, r0 = tj * P + (lj0 + 16 * b) / W;      // wave-uniform: is the block live at all
            nb += (c0 < C && r0 < R && nb == b) ? 1 : 0;
        }
        ev_d4 acc[2][2];
        prd_tile_dots<VEC>(pa, la, pb, lb, D, g, nb, acc);
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int lj = lj0 + 16 * b + col;
            const double cq = lb[b] ? cn[rq[b]] : 0.0;
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int li = li0 + 16 * a + g + 4 * k;
                    const double t = 2.0 * acc[a][b][k];
                    tile[li * PRD_PITCH + lj] = lb[b] ? cq - t : qnan;
                }
        }
        __syncthreads();
        double best = 0.0;
        int32_t idx = C;      // nothing comparable yet
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const double v = tile[srow * PRD_PITCH + 16 * part + j];
            const bool take = v == v && (idx == C || v < best);
            best = take ? v : best;
            idx = take ? pc0 + j : idx;
        }
        sbest[threadIdx.x] = best;
        sidx[threadIdx.x] = idx;
        __syncthreads();      // the tile is free for the next trip; the parts are visible
        const int r = tj * P + pseg;
        if (pc0 == 0 && r < R) {      // the first part of a run's segment takes the others, ascending
            for (int p = 1; p < W / 16; ++p) {
                const double v = sbest[threadIdx.x + p];
                const int32_t i = sidx[threadIdx.x + p];
                const bool take = i != C && (idx == C || v < best);
                best = take ? v : best;
                idx = take ? i : idx;
            }
            if (gu < U.n) assign[(int64_t)r * U.n + gu] = row_ok ? idx : C;
        }
        // sbest / sidx are written again only after the next trip's first barrier, which every merging lane reaches after these reads
    }
}

// ---- counts ----------------------------------------------------------------------------------------------------------------------------------------------
// Workgroup r: hist[r][side][c] = the rows of the side with assign[r][u] == c; column C: every other row, and every row whose norm is not finite whatever its entry.
// Integer counts in LDS (integer atomics: any order gives the same counts).
__global__ __launch_bounds__(256) void eval_prd_count_kernel(const int32_t* __restrict__ assign, const double* __restrict__ norms_a, const double* __restrict__ norms_b,
                                                             uint32_t na, uint32_t n, int C, int32_t* __restrict__ hist) {
    __shared__ int32_t h[2 * (PRD_MAX_C + 1)];
    const int r = blockIdx.x;
    for (int i = threadIdx.x; i < 2 * (PRD_MAX_C + 1); i += 256) h[i] = 0;
    __syncthreads();
    const int32_t* a = assign + (int64_t)r * n;
    for (uint32_t u = threadIdx.x; u < n; u += 256) {
        const int side = u < na ? 0 : 1;
        const bool ok = prd_finite(side ? norms_b[u - na] : norms_a[u]);
        const int32_t c = a[u];
        const int slot = (ok && (uint32_t)c < (uint32_t)C) ? c : C;
        atomicAdd(&h[side * (PRD_MAX_C + 1) + slot], 1);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * (C + 1); i += 256) {
        const int side = i / (C + 1), c = i % (C + 1);
        hist[((int64_t)r * 2 + side) * (C + 1) + c] = h[side * (PRD_MAX_C + 1) + c];
    }
}

// ---- update ----------------------------------------------------------------------------------------------------------------------------------------------
// The sums as a GEMM with the contraction over the union's rows, as eval_moments_kernel has it.  Workgroup (tj, ti, s) owns the 64 x 64 tile (packed rows q = r C + c
// 64 ti .., features 64 tj ..) of slab s's partial; wave w the 32 x 32 quarter (w >> 1, w & 1).  The A operand of rows q0 .. q0 + 15 is the selector
// assign[r(q)][u] == c(q) as 1.0 / 0.0, formed in registers (a product of it with an fp32 value is exact); the B operand is x[u][j0 + (l & 15)].  u = the slab's
// rows ascending, four per instruction.  A row past the slab, a column past D and a row whose norm is not finite (0 * NaN) are loaded as zeros.
__global__ __launch_bounds__(256) void eval_prd_sums_kernel(PrdUnion U, const double* __restrict__ norms_a, const double* __restrict__ norms_b,
                                                            const int32_t* __restrict__ assign, int D, int C, int Q, uint32_t slab, double* __restrict__ ws) {
    const int tj = blockIdx.x, ti = blockIdx.y, s = blockIdx.z;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane & 15, g = lane >> 4;
    const int i0 = ti * PRD_TILE + (wave >> 1) * 32, j0 = tj * PRD_TILE + (wave & 1) * 32;
    if (i0 >= Q) return;      // no barrier below
    ev_d4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = ev_d4{0.0, 0.0, 0.0, 0.0};
    const int32_t* ar[2];
    int32_t ac[2];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        const int q = i0 + 16 * a + col;
        const bool live = q < Q;
        ar[a] = assign + (int64_t)(live ? q / C : 0) * U.n;
        ac[a] = live ? q % C : -1;      // a row past Q selects nothing; nor does an entry outside [0, C), "unassigned" among them
    }
    const int cb[2] = {j0 + col, j0 + 16 + col};
    const bool vb[2] = {cb[0] < D, cb[1] < D};
    const uint64_t lo = (uint64_t)s * slab;
    const uint64_t hi = lo + slab < (uint64_t)U.n ? lo + slab : (uint64_t)U.n;
    for (uint64_t u0 = lo; u0 < hi; u0 += 16) {      // four instructions' rows per trip, all loads first
        double A[4][2], B[4][2];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint64_t u = u0 + 4 * k + g;
            bool rv = u < hi;
            const uint32_t uu = rv ? (uint32_t)u : (uint32_t)lo;
            rv = rv && prd_finite(uu < U.na ? norms_a[uu] : norms_b[uu - U.na]);
            const float* xr = prd_row(U, uu);
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                const int32_t e = ar[a][uu];
                A[k][a] = (rv && ac[a] >= 0 && e == ac[a]) ? 1.0 : 0.0;
            }
#pragma unroll
            for (int b = 0; b < 2; ++b) B[k][b] = (rv && vb[b]) ? (double)xr[cb[b]] : 0.0;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b) acc[a][b] = ev_mfma(A[k][a], B[k][b], acc[a][b]);
    }
    double* o = ws + (int64_t)s * Q * D;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int q = i0 + 16 * a + g + 4 * k, d = j0 + 16 * b + col;
                if (q < Q && d < D) o[(int64_t)q * D + d] = acc[a][b][k];
            }
}

// cent[q][d] = (((ws[0] + ws[1]) + ws[2]) + ...)[q][d] / count[q] where count[q] = hist[r][0][c] + hist[r][1][c] > 0; an empty cluster keeps its centroid.
__global__ __launch_bounds__(256) void eval_prd_fold_kernel(const double* __restrict__ ws, const int32_t* __restrict__ hist, int D, int C, int Q, int S,
                                                            double* __restrict__ cent) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)Q * D) return;
    const int q = (int)(i / D);
    const int r = q / C, c = q % C;
    const int64_t count = (int64_t)hist[((int64_t)r * 2 + 0) * (C + 1) + c] + (int64_t)hist[((int64_t)r * 2 + 1) * (C + 1) + c];
    if (count <= 0) return;
    double s = ws[i];
    for (int k = 1; k < S; ++k) s += ws[(int64_t)k * Q * D + i];
    cent[i] = s / (double)count;
}

static bool prd_misaligned(const void* q, uintptr_t a) { return reinterpret_cast<uintptr_t>(q) % a != 0; }

// The row slabs of an update: what the caller forces (1 .. 64), or — 0 — as many as bring the output tiles to 1024 workgroups (four per CU on 256 CUs: measured at
// the workload's size, DESIGN §18, 8 slabs of 128 tiles take 0.78 ms where 4 take 1.21), at most one per 64 rows.  From (n, R C, D) alone, never from the device.
static int prd_splits(int64_t n, int64_t Q, int D, int row_splits) {
    if (row_splits != 0) return row_splits;
    const int64_t tiles = ((Q + PRD_TILE - 1) / PRD_TILE) * ((D + PRD_TILE - 1) / PRD_TILE), nrt = (n + PRD_TILE - 1) / PRD_TILE;
    int64_t S = 1024 / tiles;
    if (S > nrt) S = nrt;
    if (S > PRD_MAX_SPLITS) S = PRD_MAX_SPLITS;
    return S < 1 ? 1 : (int)S;
}

// rows per slab: ceil(n / S) rounded up to the 16 rows of a trip, so that a slab starts on a trip's boundary
static uint32_t prd_slab(int64_t n, int S) { return (uint32_t)((((n + S - 1) / S) + 15) / 16 * 16); }

static const char* prd_shape(const float* fa, int64_t sa, int64_t na, const float* fb, int64_t sb, int64_t nb, int D, int C, int R) {
    if (!fa || !fb || prd_misaligned(fa, 4) || prd_misaligned(fb, 4)) return "null or misaligned feature pointer";
    if (D < 1 || D > PRD_MAX_D) return "1 <= D <= 4096 features";
    if (na < 1 || nb < 1 || na + nb > 0x7fffffffll) return "1 <= na, nb and na + nb < 2^31 rows";
    if (sa < D || sb < D) return "a row stride is smaller than the row";
    if (C < 1 || C > PRD_MAX_C || C > na + nb) return "1 <= C <= 64 clusters and C <= na + nb";
    if (R < 1 || R > PRD_MAX_R) return "1 <= R <= 64 runs";
    return nullptr;
}

static PrdUnion prd_union(const float* fa, int64_t sa, int64_t na, const float* fb, int64_t sb, int64_t nb) {
    PrdUnion U;
    U.fa = fa; U.fb = fb; U.sa = sa; U.sb = sb; U.na = (uint32_t)na; U.n = (uint32_t)(na + nb);
    return U;
}

}  // namespace dcv

using namespace dcv;

extern "C" {

int dcv_eval_prd_seed(const float* fa, int64_t stride_a, int64_t na, const float* fb, int64_t stride_b, int64_t nb, int D, int C, int R, uint64_t seed, double* cent,
                      void* stream) {
    const char* why = prd_shape(fa, stride_a, na, fb, stride_b, nb, D, C, R);
    if (why) return fail(DCV_EINVAL, "eval_prd_seed: %s (na %lld, nb %lld, D %d, C %d, R %d)", why, (long long)na, (long long)nb, D, C, R);
    if (!cent || prd_misaligned(cent, 8)) return fail(DCV_EINVAL, "eval_prd_seed: null or misaligned centroids");
    const uint64_t key = seed + DCV_EVAL_PRD_SALT;
    hipLaunchKernelGGL(eval_prd_seed_kernel, dim3((unsigned)(R * C)), dim3(256), 0, static_cast<hipStream_t>(stream), prd_union(fa, stride_a, na, fb, stride_b, nb), D, C,
                       clip_perm_half_bits(na + nb), (uint32_t)key, (uint32_t)(key >> 32), cent);
    DCV_LAUNCH_CHECK();
    return DCV_OK;
}

size_t dcv_eval_prd_assign_workspace_bytes(int C, int R) {
    if (C < 1 || C > PRD_MAX_C || R < 1 || R > PRD_MAX_R) return 0;
    return (size_t)C * (size_t)R * sizeof(double);
}

int dcv_eval_prd_assign(const float* fa, int64_t stride_a, int64_t na, const float* fb, int64_t stride_b, int64_t nb, const double* norms_a, const double* norms_b, int D,
                        const double* cent, int C, int R, int32_t* assign, void* workspace, size_t workspace_bytes, void* stream) {
    const char* why = prd_shape(fa, stride_a, na, fb, stride_b, nb, D, C, R);
    if (why) return fail(DCV_EINVAL, "eval_prd_assign: %s (na %lld, nb %lld, D %d, C %d, R %d)", why, (long long)na, (long long)nb, D, C, R);
    if (!norms_a || !norms_b || !cent || !assign || !workspace || prd_misaligned(norms_a, 8) || prd_misaligned(norms_b, 8) || prd_misaligned(cent, 8) ||
        prd_misaligned(assign, 4) || prd_misaligned(workspace, 8))
        return fail(DCV_EINVAL, "eval_prd_assign: null or misaligned pointer");
    const size_t need = dcv_eval_prd_assign_workspace_bytes(C, R);
    if (workspace_bytes < need) return fail(DCV_EWORKSPACE, "eval_prd_assign: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    const int64_t n = na + nb;
    const int Q = R * C;
    hipStream_t st = static_cast<hipStream_t>(stream);
    double* cn = static_cast<double*>(workspace);
    hipLaunchKernelGGL(eval_prd_cn_kernel, dim3((unsigned)((Q + 255) / 256)), dim3(256), 0, st, cent, Q, D, cn);
    DCV_LAUNCH_CHECK();
    const int64_t nrt = (n + PRD_TILE - 1) / PRD_TILE;
    const int W = C <= 16 ? 16 : (C <= 32 ? 32 : 64);      // columns per run
    const int G = (R + PRD_TILE / W - 1) / (PRD_TILE / W);      // column tiles
    int64_t RS = 512 / nrt;      // shares of the column tiles: enough workgroups for two per CU where the row tiles alone are few
    if (RS > G) RS = G;
    if (RS < 1) RS = 1;
    const dim3 grid((unsigned)nrt, (unsigned)RS);
    const PrdUnion U = prd_union(fa, stride_a, na, fb, stride_b, nb);
    const bool vec = D % 4 == 0 && stride_a % 4 == 0 && stride_b % 4 == 0 && !prd_misaligned(fa, 16) && !prd_misaligned(fb, 16) && !prd_misaligned(cent, 16);
    if (vec) hipLaunchKernelGGL((eval_prd_assign_kernel<true>), grid, dim3(256), 0, st, U, norms_a, norms_b, D, cent, cn, C, R, W, (int)RS, assign);
    else hipLaunchKernelGGL((eval_prd_assign_kernel<false>), grid, dim3(256), 0, st, U, norms_a, norms_b, D, cent, cn, C, R, W, (int)RS, assign);
    DCV_LAUNCH_CHECK();
    return DCV_OK;
}

int dcv_eval_prd_count(const int32_t* assign, const double* norms_a, int64_t na, const double* norms_b, int64_t nb, int C, int R, int32_t* hist, void* stream) {
    if (!assign || !norms_a || !norms_b || !hist || prd_misaligned(assign, 4) || prd_misaligned(norms_a, 8) || prd_misaligned(norms_b, 8) || prd_misaligned(hist, 4))
        return fail(DCV_EINVAL, "eval_prd_count: null or misaligned pointer");
    if (na < 1 || nb < 1 || na + nb > 0x7fffffffll) return fail(DCV_EINVAL, "eval_prd_count: 1 <= na, nb and na + nb < 2^31 rows (got %lld, %lld)", (long long)na, (long long)nb);
    if (C < 1 || C > PRD_MAX_C || R < 1 || R > PRD_MAX_R) return fail(DCV_EINVAL, "eval_prd_count: 1 <= C <= %d, 1 <= R <= %d (got %d, %d)", PRD_MAX_C, PRD_MAX_R, C, R);
    hipLaunchKernelGGL(eval_prd_count_kernel, dim3((unsigned)R), dim3(256), 0, static_cast<hipStream_t>(stream), assign, norms_a, norms_b, (uint32_t)na, (uint32_t)(na + nb), C,
                       hist);
    DCV_LAUNCH_CHECK();
    return DCV_OK;
}

size_t dcv_eval_prd_update_workspace_bytes(int64_t n, int D, int C, int R, int row_splits) {
    if (n < 1 || n > 0x7fffffffll || D < 1 || D > PRD_MAX_D || C < 1 || C > PRD_MAX_C || R < 1 || R > PRD_MAX_R || row_splits < 0 || row_splits > PRD_MAX_SPLITS) return 0;
    return (size_t)prd_splits(n, (int64_t)R * C, D, row_splits) * (size_t)R * (size_t)C * (size_t)D * sizeof(double);
}

int dcv_eval_prd_update(const float* fa, int64_t stride_a, int64_t na, const float* fb, int64_t stride_b, int64_t nb, const double* norms_a, const double* norms_b,
                        const int32_t* assign, int D, int C, int R, int row_splits, double* cent, int32_t* hist, void* workspace, size_t workspace_bytes, void* stream) {
    const char* why = prd_shape(fa, stride_a, na, fb, stride_b, nb, D, C, R);
    if (why) return fail(DCV_EINVAL, "eval_prd_update: %s (na %lld, nb %lld, D %d, C %d, R %d)", why, (long long)na, (long long)nb, D, C, R);
    if (!norms_a || !norms_b || !assign || !cent || !hist || !workspace || prd_misaligned(norms_a, 8) || prd_misaligned(norms_b, 8) || prd_misaligned(assign, 4) ||
        prd_misaligned(cent, 8) || prd_misaligned(hist, 4) || prd_misaligned(workspace, 8))
        return fail(DCV_EINVAL, "eval_prd_update: null or misaligned pointer");
    if (row_splits < 0 || row_splits > PRD_MAX_SPLITS) return fail(DCV_EINVAL, "eval_prd_update: 0 <= row_splits <= %d (got %d)", PRD_MAX_SPLITS, row_splits);
    const int64_t n = na + nb;
    const size_t need = dcv_eval_prd_update_workspace_bytes(n, D, C, R, row_splits);
    if (workspace_bytes < need) return fail(DCV_EWORKSPACE, "eval_prd_update: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    const int Q = R * C;
    const int S = prd_splits(n, Q, D, row_splits);
    hipStream_t st = static_cast<hipStream_t>(stream);
    double* ws = static_cast<double*>(workspace);
    hipLaunchKernelGGL(eval_prd_count_kernel, dim3((unsigned)R), dim3(256), 0, st, assign, norms_a, norms_b, (uint32_t)na, (uint32_t)n, C, hist);
    DCV_LAUNCH_CHECK();
    const dim3 grid((unsigned)((D + PRD_TILE - 1) / PRD_TILE), (unsigned)((Q + PRD_TILE - 1) / PRD_TILE), (unsigned)S);
    hipLaunchKernelGGL(eval_prd_sums_kernel, grid, dim3(256), 0, st, prd_union(fa, stride_a, na, fb, stride_b, nb), norms_a, norms_b, assign, D, C, Q, prd_slab(n, S), ws);
    DCV_LAUNCH_CHECK();
    hipLaunchKernelGGL(eval_prd_fold_kernel, dim3((unsigned)(((int64_t)Q * D + 255) / 256)), dim3(256), 0, st, ws, hist, D, C, Q, S, cent);
    DCV_LAUNCH_CHECK();
    return DCV_OK;
}

}  // extern "C"
