// LeCam regularisation of the discriminators, fp32 logits, gfx950: the anchors (an EMA of each discriminator's mean logit on the real and on the fake
// batch), the warm-up switch, the regulariser's value and its gradient all stay on the device.  Two launches per iteration: lecam_sums_kernel (the batch sums, which
// the caller may all-reduce) and lecam_apply_kernel (folds the regulariser into the loss values and stored gradients dcv_gan_loss left, then moves the anchors).
// One workgroup per discriminator, every sum in ONE fixed order (256 lanes, then an LDS tree), no atomics: the same inputs give the same bits.
#include "dcv_common.h"

namespace dcv {

// Every operation of this file is rounded on its own, never fused into a multiply-add: hipcc contracts a * b + c by default, and the specification (the numpy
// restatement in tests/test_lecam_cpu.py reproduces every bit) is mul, round, add, round.
#pragma clang fp contract(off)

static const int LECAM_MAX_DIS = 8;
static const int64_t LECAM_MAX_N = 1 << 24;

struct LecamArgs {      // the caller's host tables, by value
    const float* yr[LECAM_MAX_DIS];
    const float* yf[LECAM_MAX_DIS];
    float* dyr[LECAM_MAX_DIS];
    float* dyf[LECAM_MAX_DIS];
    float* loss[LECAM_MAX_DIS];
    int32_t nr[LECAM_MAX_DIS], nf[LECAM_MAX_DIS];
};

// The normative order above the lanes: p[l] += p[l + s] for s = 128 .. 1; every lane returns p[0].  A step's readers (l + s >= s) are not its writers (l < s).
__device__ __forceinline__ double lecam_tree(double v, double* p) {
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

__global__ __launch_bounds__(256) void lecam_sums_kernel(LecamArgs a, double* __restrict__ sums) {
    __shared__ double p[256];
    const int k = blockIdx.x;
    const float* __restrict__ yr = a.yr[k];
    const float* __restrict__ yf = a.yf[k];
    const int nr = a.nr[k], nf = a.nf[k];
    double s = 0.0;
    for (int i = threadIdx.x; i < nr; i += 256) s += (double)yr[i];
    const double sr = lecam_tree(s, p);
    s = 0.0;
    for (int i = threadIdx.x; i < nf; i += 256) s += (double)yf[i];
    const double sf = lecam_tree(s, p);
    if (threadIdx.x == 0) {
        double* o = sums + 4 * k;
        o[0] = sr; o[1] = (double)nr; o[2] = sf; o[3] = (double)nf;
    }
}

__global__ __launch_bounds__(256) void lecam_apply_kernel(LecamArgs a, const double* __restrict__ sums, int32_t* __restrict__ state, double decay, int start,
                                                          double weight, int one_sided, float* __restrict__ reg) {
    __shared__ double p[256];
    const int k = blockIdx.x;
    int32_t* st = state + k * DCV_LECAM_STATE_WORDS;
    // the state as it is BEFORE this call: lane 0 writes it only after both trees (their barriers order these reads first)
    const float aR = __builtin_bit_cast(float, st[DCV_LECAM_ANCHOR_REAL]), aF = __builtin_bit_cast(float, st[DCV_LECAM_ANCHOR_FAKE]);
    const int32_t U = st[DCV_LECAM_UPDATES];
    const bool active = U >= (start > 1 ? start : 1);
    const int nr = a.nr[k], nf = a.nf[k];
    const float* yr = a.yr[k];
    const float* yf = a.yf[k];
    float* dyr = a.dyr[k];
    float* dyf = a.dyf[k];
    const float cr = (float)(2.0 * weight / (double)nr), cf = (float)(2.0 * weight / (double)nf);
    double s = 0.0;
    for (int i = threadIdx.x; i < nr; i += 256) {
        float d = yr[i] - aF;
        if (one_sided) d = d < 0.f ? 0.f : d;      // a NaN stays a NaN
        s += (double)d * (double)d;
        if (active) {
            const float t = cr * d;
            dyr[i] = dyr[i] + t;
        }
    }
    const double Sd = lecam_tree(s, p);
    s = 0.0;
    for (int i = threadIdx.x; i < nf; i += 256) {
        float e = aR - yf[i];
        if (one_sided) e = e < 0.f ? 0.f : e;
        s += (double)e * (double)e;
        if (active) {
            const float t = cf * e;
            dyf[i] = dyf[i] - t;
        }
    }
    const double Se = lecam_tree(s, p);
    if (threadIdx.x != 0) return;
    const double qd = Sd / (double)nr, qe = Se / (double)nf;
    const double R = qd + qe;
    const float r = (float)(weight * R);
    if (active) *a.loss[k] = *a.loss[k] + r;
    reg[k] = active ? r : 0.f;
    st[DCV_LECAM_ACTIVE] = active ? 1 : 0;
    const double* sm = sums + 4 * k;
    const double mr = sm[0] / sm[1], mf = sm[2] / sm[3];
    if (!(__builtin_isfinite(mr) && __builtin_isfinite(mf))) return;      // a batch with an inf / NaN logit (or an empty one) teaches the anchors nothing
    float nR, nF;
    if (U == 0) {
        nR = (float)mr; nF = (float)mf;
    } else {
        const double w = 1.0 - decay;
        const double tr0 = (double)aR * decay, tr1 = mr * w;
        const double tf0 = (double)aF * decay, tf1 = mf * w;
        nR = (float)(tr0 + tr1); nF = (float)(tf0 + tf1);
    }
    st[DCV_LECAM_ANCHOR_REAL] = __builtin_bit_cast(int32_t, nR);
    st[DCV_LECAM_ANCHOR_FAKE] = __builtin_bit_cast(int32_t, nF);
    st[DCV_LECAM_UPDATES] = U + 1;
}

// Every check comes before the launch.  dy / loss are looked at for dcv_lecam_apply only.
static int lecam_pack(const char* who, int n_dis, const float* const* y_real, const float* const* y_fake, const int64_t* n_real, const int64_t* n_fake,
                      float* const* loss, float* const* dy_real, float* const* dy_fake, bool apply, LecamArgs* a) {
    if (n_dis < 1 || n_dis > LECAM_MAX_DIS) return fail(DCV_EINVAL, "%s: 1 <= n_dis <= %d (got %d)", who, LECAM_MAX_DIS, n_dis);
    if (!y_real || !y_fake || !n_real || !n_fake || (apply && (!loss || !dy_real || !dy_fake))) return fail(DCV_EINVAL, "%s: null table", who);
    memset(a, 0, sizeof(*a));
    for (int k = 0; k < n_dis; ++k) {
        if (n_real[k] < 1 || n_real[k] > LECAM_MAX_N || n_fake[k] < 1 || n_fake[k] > LECAM_MAX_N)
            return fail(DCV_EINVAL, "%s: 1 <= n <= 2^24 logits per tensor (discriminator %d: %lld real, %lld fake)", who, k, (long long)n_real[k], (long long)n_fake[k]);
        const void* ptrs[5] = {y_real[k], y_fake[k], apply ? loss[k] : y_real[k], apply ? dy_real[k] : y_real[k], apply ? dy_fake[k] : y_real[k]};
        for (const void* q : ptrs)
            if (!q || reinterpret_cast<uintptr_t>(q) % 4) return fail(DCV_EINVAL, "%s: null or misaligned tensor (discriminator %d)", who, k);
        a->yr[k] = y_real[k]; a->yf[k] = y_fake[k];
        a->nr[k] = (int32_t)n_real[k]; a->nf[k] = (int32_t)n_fake[k];
        if (apply) { a->loss[k] = loss[k]; a->dyr[k] = dy_real[k]; a->dyf[k] = dy_fake[k]; }
    }
    return DCV_OK;
}

}  // namespace dcv

using namespace dcv;

extern "C" {

int dcv_lecam_sums(int n_dis, const float* const* y_real, const float* const* y_fake, const int64_t* n_real, const int64_t* n_fake, double* sums, void* stream) {
    LecamArgs a;
    const int rc = lecam_pack("lecam_sums", n_dis, y_real, y_fake, n_real, n_fake, nullptr, nullptr, nullptr, false, &a);
    if (rc != DCV_OK) return rc;
    if (!sums || reinterpret_cast<uintptr_t>(sums) % 8) return fail(DCV_EINVAL, "lecam_sums: sums must be n_dis x 4 doubles on an 8-byte boundary");
    hipLaunchKernelGGL(lecam_sums_kernel, dim3((unsigned)n_dis), dim3(256), 0, static_cast<hipStream_t>(stream), a, sums);
    DCV_LAUNCH_CHECK();
    return DCV_OK;
}

int dcv_lecam_apply(int n_dis, const float* const* y_real, const float* const* y_fake, const int64_t* n_real, const int64_t* n_fake, const double* sums,
                    int32_t* state, double decay, int start, double weight, int one_sided, float* const* loss, float* const* dy_real, float* const* dy_fake,
                    float* reg, void* stream) {
    LecamArgs a;
    const int rc = lecam_pack("lecam_apply", n_dis, y_real, y_fake, n_real, n_fake, loss, dy_real, dy_fake, true, &a);
    if (rc != DCV_OK) return rc;
    if (!sums || reinterpret_cast<uintptr_t>(sums) % 8) return fail(DCV_EINVAL, "lecam_apply: sums must be n_dis x 4 doubles on an 8-byte boundary");
    if (!state || !reg || reinterpret_cast<uintptr_t>(state) % 4 || reinterpret_cast<uintptr_t>(reg) % 4) return fail(DCV_EINVAL, "lecam_apply: null or misaligned state / reg");
    if (!(decay >= 0.0 && decay <= 1.0)) return fail(DCV_EINVAL, "lecam_apply: decay must be in [0, 1]");
    if (!(weight >= 0.0) || !__builtin_isfinite(weight)) return fail(DCV_EINVAL, "lecam_apply: weight must be finite and >= 0");
    hipLaunchKernelGGL(lecam_apply_kernel, dim3((unsigned)n_dis), dim3(256), 0, static_cast<hipStream_t>(stream), a, sums, state, decay, start, weight,
                       one_sided ? 1 : 0, reg);
    DCV_LAUNCH_CHECK();
    return DCV_OK;
}

}  // extern "C"
