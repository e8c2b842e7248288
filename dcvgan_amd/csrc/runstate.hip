// RunState, gfx950: every state tensor of a training run as 32-bit words.  dcv_state_pack_multi copies the tensors into a caller-owned arena and
// leaves a 128-bit digest of each, dcv_state_unpack_multi copies arena segments back, dcv_state_digest_multi forms the digests alone.  Up to RS_MT tensors per
// launch, with the block mapping of the optimiser kernels' multi-tensor table, kept local to this file: a block is 256 threads and 4096 dwords.
//
// The digest of a tensor of n dwords w[0 .. n): h_i = splitmix64-finaliser(i * 0x9E3779B97F4A7C15 + w[i]) mod 2^64; the pair (sum of h_i mod 2^64, xor of h_i).
// Both combines are commutative and exact, so the bits depend on neither the traversal nor the schedule: a block leaves its partial pair in the workspace
// (rs_kernel) and one block per tensor folds the tensor's partials (rs_final_kernel).  No atomics.  runstate.digest_host is the numpy mirror.
#include <algorithm>

#include "dcv_common.h"

namespace dcv {

static const int RS_MT = 24;                              // tensors per launch, as ADAM_MT
static const int RS_BLOCK = 4096;                         // dwords per block, as MT_BLOCK
static const int64_t RS_MAX_DWORDS = (int64_t)1 << 32;    // a tensor's dword index is hashed as a 32-bit quantity's worth of positions

struct RsBlocks {
    int32_t first_block[RS_MT + 1];      // prefix sum of the tensors' block counts
};
struct RsPack {
    const uint32_t* src[RS_MT];
    uint32_t* dst[RS_MT];                // (digest: unused)
    int64_t n[RS_MT];                    // dwords
    RsBlocks tab;
};

enum RsMode { RS_PACK, RS_UNPACK, RS_DIGEST };

__device__ __forceinline__ uint64_t rs_hash(uint64_t i, uint32_t w) {
    uint64_t z = i * 0x9E3779B97F4A7C15ull + (uint64_t)w;
    z ^= z >> 30;
    z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27;
    z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}

// (sum, xor) over the block's 256 lanes; lane 0 holds the result.  A step's readers (l + s >= s) are not its writers (l < s).
__device__ __forceinline__ void rs_tree(uint64_t& s, uint64_t& x, uint64_t* ps, uint64_t* px) {
    const int l = threadIdx.x;
    ps[l] = s; px[l] = x;
    __syncthreads();
#pragma unroll
    for (int d = 128; d >= 1; d >>= 1) {
        if (l < d) { ps[l] += ps[l + d]; px[l] ^= px[l + d]; }
        __syncthreads();
    }
    s = ps[0]; x = px[0];
}

__device__ __forceinline__ bool rs_aligned16(const void* a, const void* b = nullptr) {
    return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15) == 0;
}

// One block: (at most) 4096 dwords of one tensor.  With every base on a 16-byte boundary four 16-byte accesses per thread and the tensor's last 1..3 dwords one
// at a time, else 16 coalesced dword accesses per thread (the digest does not care who visits which dword).  RS_PACK's last block of a tensor also writes the
// zero dwords up to the next 16-byte boundary of the arena segment.
template <RsMode MODE>
__global__ __launch_bounds__(256) void rs_kernel(const RsPack k, int nt, uint64_t* __restrict__ partial) {
    __shared__ uint64_t ps[256], px[256];
    int t = 0;
    while (t + 1 < nt && (int)blockIdx.x >= k.tab.first_block[t + 1]) ++t;
    const int blk = (int)blockIdx.x - k.tab.first_block[t];
    const uint32_t* __restrict__ src = k.src[t];
    uint32_t* __restrict__ dst = MODE == RS_DIGEST ? nullptr : k.dst[t];
    const int64_t n = k.n[t];
    const int64_t base = (int64_t)blk * RS_BLOCK;
    uint64_t s = 0, x = 0;
    auto one = [&](int64_t j) {
        const uint32_t w = src[j];
        if (MODE != RS_DIGEST) dst[j] = w;
        if (MODE != RS_UNPACK) { const uint64_t h = rs_hash((uint64_t)j, w); s += h; x ^= h; }
    };
    if (rs_aligned16(src, dst)) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t i = base + (int64_t)(q * 256 + (int)threadIdx.x) * 4;
            if (i + 4 <= n) {
                const uint4 v = *reinterpret_cast<const uint4*>(src + i);
                if (MODE != RS_DIGEST) *reinterpret_cast<uint4*>(dst + i) = v;
                if (MODE != RS_UNPACK) {
                    const uint64_t h0 = rs_hash((uint64_t)i, v.x), h1 = rs_hash((uint64_t)i + 1, v.y), h2 = rs_hash((uint64_t)i + 2, v.z), h3 = rs_hash((uint64_t)i + 3, v.w);
                    s += (h0 + h1) + (h2 + h3);
                    x ^= (h0 ^ h1) ^ (h2 ^ h3);
                }
            } else {
                for (int64_t j = i; j < n; ++j) one(j);
            }
        }
    } else {
#pragma unroll 4
        for (int e = 0; e < 16; ++e) {
            const int64_t j = base + e * 256 + (int)threadIdx.x;
            if (j >= n) break;
            one(j);
        }
    }
    if (MODE == RS_PACK && base + RS_BLOCK >= n) {      // the tensor's last block: the segment's padding
        const int64_t j = n + (int)threadIdx.x;
        if (threadIdx.x < 3 && j < ((n + 3) & ~(int64_t)3)) dst[j] = 0u;
    }
    if (MODE == RS_UNPACK) return;
    rs_tree(s, x, ps, px);
    if (threadIdx.x == 0) {
        partial[2 * (int64_t)blockIdx.x] = s;
        partial[2 * (int64_t)blockIdx.x + 1] = x;
    }
}

// One block per tensor of the table: the tensor's partial pairs, folded.  A tensor without dwords has no partials and the digest (0, 0).
__global__ __launch_bounds__(256) void rs_final_kernel(const RsBlocks tab, const uint64_t* __restrict__ partial, uint64_t* __restrict__ digests) {
    __shared__ uint64_t ps[256], px[256];
    const int t = blockIdx.x;
    const int a = tab.first_block[t], b = tab.first_block[t + 1];
    uint64_t s = 0, x = 0;
    for (int j = a + (int)threadIdx.x; j < b; j += 256) { s += partial[2 * (int64_t)j]; x ^= partial[2 * (int64_t)j + 1]; }
    rs_tree(s, x, ps, px);
    if (threadIdx.x == 0) { digests[2 * t] = s; digests[2 * t + 1] = x; }
}

static int64_t rs_blocks(int64_t dwords) { return (dwords + RS_BLOCK - 1) / RS_BLOCK; }
static int64_t rs_padded(int64_t dwords) { return (dwords + 3) & ~(int64_t)3; }

// Every check of the sizes and of the caller's tensors; *total_blocks is the workspace's size in partial pairs.
static int rs_check_sizes(const char* who, int n_tensors, const int64_t* dwords, int64_t* total_blocks) {
    if (n_tensors < 0) return fail(DCV_EINVAL, "%s: n_tensors < 0", who);
    if (n_tensors > 0 && !dwords) return fail(DCV_EINVAL, "%s: null table", who);
    int64_t blocks = 0;
    for (int t = 0; t < n_tensors; ++t) {
        if (dwords[t] < 0 || dwords[t] >= RS_MAX_DWORDS)
            return fail(DCV_EINVAL, "%s: tensor %d has %lld dwords: 0 <= dwords < 2^32", who, t, (long long)dwords[t]);
        blocks += rs_blocks(dwords[t]);
    }
    *total_blocks = blocks;
    return DCV_OK;
}
static int rs_check_tensors(const char* who, int n_tensors, const void* const* p, const int64_t* dwords) {
    if (n_tensors > 0 && !p) return fail(DCV_EINVAL, "%s: null table", who);
    for (int t = 0; t < n_tensors; ++t)
        if (dwords[t] > 0 && (!p[t] || reinterpret_cast<uintptr_t>(p[t]) % 4)) return fail(DCV_EINVAL, "%s: tensor %d is null or not on a 4-byte boundary", who, t);
    return DCV_OK;
}
// The arena: on a 16-byte boundary; segments start on 16-byte boundaries, ascend, do not overlap (padding included) and end inside it.
static int rs_check_arena(const char* who, int n_tensors, const int64_t* dwords, const void* arena, int64_t arena_dwords, const int64_t* offsets) {
    if (n_tensors == 0) return DCV_OK;
    if (!arena || reinterpret_cast<uintptr_t>(arena) % 16 || arena_dwords < 0) return fail(DCV_EINVAL, "%s: the arena must be on a 16-byte boundary", who);
    if (!offsets) return fail(DCV_EINVAL, "%s: null table", who);
    int64_t end = 0;
    for (int t = 0; t < n_tensors; ++t) {
        if (offsets[t] % 4 || offsets[t] < end)
            return fail(DCV_EINVAL, "%s: segment %d starts at dword %lld: offsets are multiples of 4 dwords, ascending, past the segment before (%lld)", who, t,
                        (long long)offsets[t], (long long)end);
        if (offsets[t] > arena_dwords || rs_padded(dwords[t]) > arena_dwords - offsets[t])
            return fail(DCV_EINVAL, "%s: segment %d (%lld dwords at %lld) ends outside the arena of %lld dwords", who, t, (long long)dwords[t], (long long)offsets[t],
                        (long long)arena_dwords);
        end = offsets[t] + rs_padded(dwords[t]);
    }
    return DCV_OK;
}
static int rs_check_digest_out(const char* who, int n_tensors, const uint64_t* digests, const void* ws, size_t ws_bytes, int64_t total_blocks) {
    if (n_tensors > 0 && (!digests || reinterpret_cast<uintptr_t>(digests) % 8)) return fail(DCV_EINVAL, "%s: digests must be n_tensors x 2 uint64 on an 8-byte boundary", who);
    const size_t need = (size_t)total_blocks * 16;
    if (need > 0 && (!ws || reinterpret_cast<uintptr_t>(ws) % 8)) return fail(DCV_EINVAL, "%s: the workspace must be on an 8-byte boundary", who);
    if (ws_bytes < need) return fail(DCV_EWORKSPACE, "%s: workspace of %zu bytes, %zu needed (dcv_state_workspace_bytes)", who, ws_bytes, need);
    return DCV_OK;
}

// Walks the tensors in tables of RS_MT: per table one rs_kernel launch over its blocks (none for a table without dwords) and, with digests, one rs_final_kernel
// launch.  Every check belongs BEFORE the call: nothing here refuses.
template <RsMode MODE, class Src, class Dst>
static int rs_run(int n_tensors, const int64_t* dwords, Src src_of, Dst dst_of, uint64_t* digests, void* ws, hipStream_t st) {
    int64_t before = 0;
    for (int t0 = 0; t0 < n_tensors; t0 += RS_MT) {
        RsPack k;
        memset(&k, 0, sizeof(k));
        const int nt = std::min(RS_MT, n_tensors - t0);
        int64_t blocks = 0;
        for (int t = 0; t < nt; ++t) {
            k.src[t] = static_cast<const uint32_t*>(src_of(t0 + t));
            k.dst[t] = static_cast<uint32_t*>(dst_of(t0 + t));
            k.n[t] = dwords[t0 + t];
            k.tab.first_block[t] = (int32_t)blocks;
            blocks += rs_blocks(dwords[t0 + t]);
        }
        k.tab.first_block[nt] = (int32_t)blocks;      // <= 24 * 2^20
        uint64_t* partial = static_cast<uint64_t*>(ws) + 2 * before;
        if (blocks > 0) {
            hipLaunchKernelGGL(rs_kernel<MODE>, dim3((unsigned)blocks), dim3(256), 0, st, k, nt, partial);
            DCV_LAUNCH_CHECK();
        }
        if (MODE != RS_UNPACK) {
            hipLaunchKernelGGL(rs_final_kernel, dim3((unsigned)nt), dim3(256), 0, st, k.tab, partial, digests + 2 * (int64_t)t0);
            DCV_LAUNCH_CHECK();
        }
        before += blocks;
    }
    return DCV_OK;
}

}  // namespace dcv

using namespace dcv;

extern "C" {

size_t dcv_state_workspace_bytes(int n_tensors, const int64_t* dwords) {
    int64_t blocks = 0;
    if (rs_check_sizes("state_workspace_bytes", n_tensors, dwords, &blocks) != DCV_OK) return 0;
    return std::max<size_t>((size_t)blocks * 16, 16);
}

int dcv_state_pack_multi(int n_tensors, const void* const* src, const int64_t* dwords, void* arena, int64_t arena_dwords, const int64_t* offsets,
                         uint64_t* digests, void* workspace, size_t workspace_bytes, void* stream) {
    int64_t blocks = 0;
    int rc = rs_check_sizes("state_pack_multi", n_tensors, dwords, &blocks);
    if (rc == DCV_OK) rc = rs_check_tensors("state_pack_multi", n_tensors, src, dwords);
    if (rc == DCV_OK) rc = rs_check_arena("state_pack_multi", n_tensors, dwords, arena, arena_dwords, offsets);
    if (rc == DCV_OK) rc = rs_check_digest_out("state_pack_multi", n_tensors, digests, workspace, workspace_bytes, blocks);
    if (rc != DCV_OK) return rc;
    uint32_t* a = static_cast<uint32_t*>(arena);
    return rs_run<RS_PACK>(n_tensors, dwords, [&](int t) { return src[t]; }, [&](int t) { return static_cast<void*>(a + offsets[t]); }, digests, workspace,
                           static_cast<hipStream_t>(stream));
}

int dcv_state_unpack_multi(int n_tensors, void* const* dst, const int64_t* dwords, const void* arena, int64_t arena_dwords, const int64_t* offsets, void* stream) {
    int64_t blocks = 0;
    int rc = rs_check_sizes("state_unpack_multi", n_tensors, dwords, &blocks);
    if (rc == DCV_OK) rc = rs_check_tensors("state_unpack_multi", n_tensors, dst, dwords);
    if (rc == DCV_OK) rc = rs_check_arena("state_unpack_multi", n_tensors, dwords, arena, arena_dwords, offsets);
    if (rc != DCV_OK) return rc;
    const uint32_t* a = static_cast<const uint32_t*>(arena);
    return rs_run<RS_UNPACK>(n_tensors, dwords, [&](int t) { return static_cast<const void*>(a + offsets[t]); }, [&](int t) { return dst[t]; }, nullptr, nullptr,
                             static_cast<hipStream_t>(stream));
}

int dcv_state_digest_multi(int n_tensors, const void* const* src, const int64_t* dwords, uint64_t* digests, void* workspace, size_t workspace_bytes, void* stream) {
    int64_t blocks = 0;
    int rc = rs_check_sizes("state_digest_multi", n_tensors, dwords, &blocks);
    if (rc == DCV_OK) rc = rs_check_tensors("state_digest_multi", n_tensors, src, dwords);
    if (rc == DCV_OK) rc = rs_check_digest_out("state_digest_multi", n_tensors, digests, workspace, workspace_bytes, blocks);
    if (rc != DCV_OK) return rc;
    return rs_run<RS_DIGEST>(n_tensors, dwords, [&](int t) { return src[t]; }, [&](int t) { return static_cast<void*>(nullptr); }, digests, workspace,
                             static_cast<hipStream_t>(stream));
}

}  // extern "C"
