// The temporal window over content statistics (vstnet.h, "Statistics window", version 113): the {n, mean, cov} records of a
// frame and of up to seven frames before it -> the record of the union of their pixels, weighted by age, with a scene-cut test
// that drops everything from before a cut.  One launch between the statistics and the factor calls; it runs once per frame and
// moves at most 8 x 32 records, so it is latency-bound: one workgroup per record, three short phases, nothing clever.
#include "common.h"

#include <cmath>

namespace {

constexpr int POOL_MAX_AGES = VST_STATS_POOL_MAX;
constexpr int POOL_MAX_N = 256;
constexpr int POOL_THREADS = 256;
constexpr int POOL_WAVES = POOL_THREADS / 64;

struct PoolArgs {                       // pointers and weights travel by value (as vst_seg_mix_logits passes its)
    const double* rec[POOL_MAX_AGES];
    double w[POOL_MAX_AGES];
};

// The sum of `v` over the workgroup, the same bits in every thread: a shuffle tree per wave, then the waves' sums from LDS in
// wave order.  `slot` = POOL_WAVES doubles of LDS; two barriers, so the slot can be reused right away.
__device__ __forceinline__ double pool_block_sum(double v, double* slot) {
#pragma clang fp contract(off)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = v + __shfl_down(v, off, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = slot[0];
#pragma unroll
    for (int k = 1; k < POOL_WAVES; ++k) s = s + slot[k];
    return s;
}

__device__ __forceinline__ void pool_copy(const double* src, double* dst, int len) {      // the bits, whatever they are
    const unsigned long long* s = reinterpret_cast<const unsigned long long*>(src);
    unsigned long long* d = reinterpret_cast<unsigned long long*>(dst);
    for (int e = threadIdx.x; e < len; e += POOL_THREADS) d[e] = s[e];
}

// Record r of every age -> record r of out.  Every decision (usable, cut, the selected set) is made from values all threads of
// the workgroup hold alike, so the branches and the barriers inside them are uniform.  The arithmetic is the header's, operation
// for operation and in increasing age (no contraction): tests/stats_window_ref.py restates it.
__global__ __launch_bounds__(POOL_THREADS) void cwct_stats_pool_kernel(PoolArgs a, int n_ages, int N, double cut,
                                                                         double* __restrict__ out, int* __restrict__ used) {
#pragma clang fp contract(off)
    __shared__ double red[POOL_WAVES];
    __shared__ double mu[POOL_MAX_N];
    __shared__ double delta[POOL_MAX_AGES][POOL_MAX_N];         // mean of age a minus the pooled mean
    const int len = 1 + N + N * N, NN = N * N;
    const size_t base = (size_t)blockIdx.x * len;
    const int tid = threadIdx.x;
    const double* p0 = a.rec[0] + base;
    double* o = out + base;

    double cnt[POOL_MAX_AGES];
    unsigned sel = 0;                                           // bit a: age a is usable (n >= 2; false for NaN and n < 0)
#pragma unroll
    for (int k = 0; k < POOL_MAX_AGES; ++k) {
        cnt[k] = k < n_ages ? a.rec[k][base] : 0.0;
        if (cnt[k] >= 2.0) sel |= 1u << k;
    }
    if (!(sel & 1u)) {                                          // nothing to pool into: the factor sees what it sees today
        pool_copy(p0, o, len);
        if (used && tid == 0) used[blockIdx.x] = 0;
        return;
    }
    if (cut > 0.0 && (sel & ~1u)) {
        double t = 0.0;
        for (int i = tid; i < N; i += POOL_THREADS) t = t + p0[1 + N + (size_t)i * N + i];
        const double limit = cut * pool_block_sum(t, red);      // cut * tr(C_0)
#pragma unroll
        for (int k = 1; k < POOL_MAX_AGES; ++k) {               // (unrolled: a.rec[k] stays a kernel argument, never an array)
            if (!((sel >> k) & 1u)) continue;                   // an unusable age is skipped: it does not stop the scan
            const double* pk = a.rec[k] + base;
            double dm = 0.0, dc = 0.0;
            for (int i = tid; i < N; i += POOL_THREADS) {
                const double d = pk[1 + i] - p0[1 + i];
                dm = dm + d * d;
            }
            for (int e = tid; e < NN; e += POOL_THREADS) {
                const double d = pk[1 + N + e] - p0[1 + N + e];
                dc = dc + d * d;
            }
            dm = pool_block_sum(dm, red);
            dc = pool_block_sum(dc, red);
            // a scene cut: this age and every older one are left out (their bits go, so the scan skips them)
            if (dm + sqrt(dc) > limit) sel &= (1u << k) - 1u;
        }
    }
    const int n_used = __popc(sel);
    if (used && tid == 0) used[blockIdx.x] = n_used;
    if (n_used == 1) {
        pool_copy(p0, o, len);
        return;
    }
    double m[POOL_MAX_AGES], M = 0.0;
#pragma unroll
    for (int k = 0; k < POOL_MAX_AGES; ++k) {
        m[k] = a.w[k] * cnt[k];
        if ((sel >> k) & 1u) M = M + m[k];
    }
    for (int i = tid; i < N; i += POOL_THREADS) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < POOL_MAX_AGES; ++k)
            if ((sel >> k) & 1u) s = s + m[k] * a.rec[k][base + 1 + i];
        mu[i] = s / M;
    }
    __syncthreads();
    for (int i = tid; i < N; i += POOL_THREADS) {
#pragma unroll
        for (int k = 0; k < POOL_MAX_AGES; ++k)
            if ((sel >> k) & 1u) delta[k][i] = a.rec[k][base + 1 + i] - mu[i];
        o[1 + i] = mu[i];
    }
    if (tid == 0) o[0] = M;
    __syncthreads();
    const double den = M - 1.0;
    for (int e = tid; e < NN; e += POOL_THREADS) {
        const int i = e / N, j = e - i * N;
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < POOL_MAX_AGES; ++k)
            if ((sel >> k) & 1u) {
                const double t = (cnt[k] - 1.0) * a.rec[k][base + 1 + N + e] + (cnt[k] * delta[k][i]) * delta[k][j];
                s = s + a.w[k] * t;
            }
        o[1 + N + e] = s / den;
    }
}

}  // namespace

int vst_cwct_stats_pool(const double* const* records_host_array, const double* weights_host, int n_ages, int n_records, int N,
                        double cut, double* out, int* used, void* stream) {
    if (!records_host_array || !weights_host || !out || ((uintptr_t)out & 7) || ((uintptr_t)used & 3)) return VST_E_ARG;
    if (n_ages < 1 || n_ages > POOL_MAX_AGES || n_records < 1 || n_records > CWCT_MAX_SLOTS || N < 1 || N > POOL_MAX_N)
        return VST_E_SHAPE;
    if (!(cut >= 0.0) || !std::isfinite(cut)) return VST_E_ARG;
    PoolArgs a;
    const uintptr_t o0 = (uintptr_t)out, bytes = (uintptr_t)n_records * (1 + N + (size_t)N * N) * sizeof(double);
    for (int k = 0; k < POOL_MAX_AGES; ++k) {
        a.rec[k] = k < n_ages ? records_host_array[k] : nullptr;
        a.w[k] = k < n_ages ? weights_host[k] : 0.0;
        if (k >= n_ages) continue;
        const uintptr_t x0 = (uintptr_t)a.rec[k];
        if (!x0 || (x0 & 7)) return VST_E_ARG;
        if (!(a.w[k] > 0.0) || !std::isfinite(a.w[k])) return VST_E_ARG;
        if (x0 < o0 + bytes && o0 < x0 + bytes) return VST_E_ARG;      // out overlaps an input
    }
    hipStream_t st = (hipStream_t)stream;
    vst_prof_scope prof(VST_KERNEL_CWCT_POOL, st);
    cwct_stats_pool_kernel<<<n_records, POOL_THREADS, 0, st>>>(a, n_ages, N, cut, out, used);
    VST_RETURN_IF_LAUNCH_FAILED();
    return VST_OK;
}
