// The temporal window over content statistics (vstnet.h, "Statistics window", versions 113, 114): the {n, mean, cov} records of a
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

// One record: the age-a record at p[a] (a < n_ages; `present` bit a clear = the age has no record for this one and counts as
// unusable, p[a] is then never read) -> o.  Both kernels below end here, so the arithmetic is one text.  Every decision (usable,
// cut, the selected set) is made from values all threads of the workgroup hold alike, so the branches and the barriers inside
// them are uniform.  The arithmetic is the header's, operation for operation and in increasing age (no contraction):
// tests/stats_window_ref.py restates it.  (Every loop over the ages is unrolled: p[k] and w[k] stay registers, never an array.)
__device__ __forceinline__ void pool_record(const double* const (&p)[POOL_MAX_AGES], const double (&w)[POOL_MAX_AGES],
                                            unsigned present, int N, double cut, double* __restrict__ o, int* used_r) {
#pragma clang fp contract(off)
    __shared__ double red[POOL_WAVES];
    __shared__ double mu[POOL_MAX_N];
    __shared__ double delta[POOL_MAX_AGES][POOL_MAX_N];         // mean of age a minus the pooled mean
    const int len = 1 + N + N * N, NN = N * N;
    const int tid = threadIdx.x;
    const double* p0 = p[0];

    double cnt[POOL_MAX_AGES];
    unsigned sel = 0;                                           // bit a: age a is usable (n >= 2; false for NaN and n < 0)
#pragma unroll
    for (int k = 0; k < POOL_MAX_AGES; ++k) {
        cnt[k] = (present >> k) & 1u ? p[k][0] : 0.0;
        if (cnt[k] >= 2.0) sel |= 1u << k;
    }
    if (!(sel & 1u)) {                                          // nothing to pool into: the factor sees what it sees today
        pool_copy(p0, o, len);
        if (used_r && tid == 0) *used_r = 0;
        return;
    }
    if (cut > 0.0 && (sel & ~1u)) {
        double t = 0.0;
        for (int i = tid; i < N; i += POOL_THREADS) t = t + p0[1 + N + (size_t)i * N + i];
        const double limit = cut * pool_block_sum(t, red);      // cut * tr(C_0)
#pragma unroll
        for (int k = 1; k < POOL_MAX_AGES; ++k) {
            if (!((sel >> k) & 1u)) continue;                   // an unusable age is skipped: it does not stop the scan
            const double* pk = p[k];
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
    if (used_r && tid == 0) *used_r = n_used;
    if (n_used == 1) {
        pool_copy(p0, o, len);
        return;
    }
    double m[POOL_MAX_AGES], M = 0.0;
#pragma unroll
    for (int k = 0; k < POOL_MAX_AGES; ++k) {
        m[k] = w[k] * cnt[k];
        if ((sel >> k) & 1u) M = M + m[k];
    }
    for (int i = tid; i < N; i += POOL_THREADS) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < POOL_MAX_AGES; ++k)
            if ((sel >> k) & 1u) s = s + m[k] * p[k][1 + i];
        mu[i] = s / M;
    }
    __syncthreads();
    for (int i = tid; i < N; i += POOL_THREADS) {
#pragma unroll
        for (int k = 0; k < POOL_MAX_AGES; ++k)
            if ((sel >> k) & 1u) delta[k][i] = p[k][1 + i] - mu[i];
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
                const double t = (cnt[k] - 1.0) * p[k][1 + N + e] + (cnt[k] * delta[k][i]) * delta[k][j];
                s = s + w[k] * t;
            }
        o[1 + N + e] = s / den;
    }
}

// Record r of every age -> record r of out: the ages line up by slot.
__global__ __launch_bounds__(POOL_THREADS) void cwct_stats_pool_kernel(PoolArgs a, int n_ages, int N, double cut,
                                                                         double* __restrict__ out, int* __restrict__ used) {
    const size_t base = (size_t)blockIdx.x * (1 + N + N * N);
    const double* p[POOL_MAX_AGES];
    unsigned present = 0;
#pragma unroll
    for (int k = 0; k < POOL_MAX_AGES; ++k) {
        p[k] = k < n_ages ? a.rec[k] + base : nullptr;
        if (k < n_ages) present |= 1u << k;
    }
    pool_record(p, a.w, present, N, cut, out + base, used ? used + blockIdx.x : nullptr);
}

struct PoolPlans {                      // the plan each age's records were reduced under (device pointers, by value)
    const LabelPlan* plan[POOL_MAX_AGES];
};

// Slot r of the NEWEST plan -> record r of out: the ages line up by LABEL.  L = plan[0]->slot_label[r]; in every older age the
// record of L sits at the slot whose slot_label is L, if that age's plan holds L at all (a miss: the age is unusable for this
// record, like n < 2).  The search stops at the age's n_slots: slot_label is zero-padded beyond it and label 0 is a legal key.
// A plan's labels are distinct, so at most one thread writes hit[a]; all threads then read the same words: uniform decisions.
__global__ __launch_bounds__(POOL_THREADS) void cwct_stats_pool_keyed_kernel(PoolArgs a, PoolPlans pl, int n_ages, int N,
                                                                               double cut, double* __restrict__ out,
                                                                               int* __restrict__ used) {
    static_assert(POOL_THREADS == POOL_MAX_AGES * CWCT_MAX_SLOTS, "one thread per (age, slot) of the key lookup");
    __shared__ int hit[POOL_MAX_AGES];
    const int r = blockIdx.x, tid = threadIdx.x;
    const int n0 = min(pl.plan[0]->n_slots, (int)gridDim.x);   // (as for the older ages below: never past max_slots)
    if (r >= n0) {                                              // a slot the newest frame never reduced: nothing to read
        if (used && tid == 0) used[r] = 0;
        return;
    }
    const int L = pl.plan[0]->slot_label[r];
    if (tid < POOL_MAX_AGES) hit[tid] = tid == 0 ? r : -1;
    __syncthreads();
    {
        const int k = tid / CWCT_MAX_SLOTS, s = tid % CWCT_MAX_SLOTS;
        if (k >= 1 && k < n_ages) {
            const LabelPlan* q = pl.plan[k];
            // (s < gridDim.x = max_slots: an age's block holds max_slots records, whatever its plan says)
            if (s < min(q->n_slots, (int)gridDim.x) && q->slot_label[s] == L) hit[k] = s;
        }
    }
    __syncthreads();
    const size_t len = 1 + N + (size_t)N * N;
    const double* p[POOL_MAX_AGES];
    unsigned present = 0;
#pragma unroll
    for (int k = 0; k < POOL_MAX_AGES; ++k) {
        const int s = k < n_ages ? hit[k] : -1;
        p[k] = s >= 0 ? a.rec[k] + (size_t)s * len : nullptr;
        if (s >= 0) present |= 1u << k;
    }
    pool_record(p, a.w, present, N, cut, out + (size_t)r * len, used ? used + r : nullptr);
}

// the checks the two entries share: VST_OK, or the status to return
int pool_args(const double* const* recs, const double* weights, int n_ages, int n_records, int N, double cut, const double* out,
              const int* used, PoolArgs& a) {
    if (!recs || !weights || !out || ((uintptr_t)out & 7) || ((uintptr_t)used & 3)) return VST_E_ARG;
    if (n_ages < 1 || n_ages > POOL_MAX_AGES || n_records < 1 || n_records > CWCT_MAX_SLOTS || N < 1 || N > POOL_MAX_N)
        return VST_E_SHAPE;
    if (!(cut >= 0.0) || !std::isfinite(cut)) return VST_E_ARG;
    const uintptr_t o0 = (uintptr_t)out, bytes = (uintptr_t)n_records * (1 + N + (size_t)N * N) * sizeof(double);
    for (int k = 0; k < POOL_MAX_AGES; ++k) {
        a.rec[k] = k < n_ages ? recs[k] : nullptr;
        a.w[k] = k < n_ages ? weights[k] : 0.0;
        if (k >= n_ages) continue;
        const uintptr_t x0 = (uintptr_t)a.rec[k];
        if (!x0 || (x0 & 7)) return VST_E_ARG;
        if (!(a.w[k] > 0.0) || !std::isfinite(a.w[k])) return VST_E_ARG;
        if (x0 < o0 + bytes && o0 < x0 + bytes) return VST_E_ARG;      // out overlaps an input
    }
    return VST_OK;
}

}  // namespace

int vst_cwct_stats_pool(const double* const* records_host_array, const double* weights_host, int n_ages, int n_records, int N,
                        double cut, double* out, int* used, void* stream) {
    PoolArgs a;
    if (int rc = pool_args(records_host_array, weights_host, n_ages, n_records, N, cut, out, used, a)) return rc;
    hipStream_t st = (hipStream_t)stream;
    vst_prof_scope prof(VST_KERNEL_CWCT_POOL, st);
    cwct_stats_pool_kernel<<<n_records, POOL_THREADS, 0, st>>>(a, n_ages, N, cut, out, used);
    VST_RETURN_IF_LAUNCH_FAILED();
    return VST_OK;
}

int vst_cwct_stats_pool_keyed(const double* const* records_host_array, const void* const* plans_host_array,
                              const double* weights_host, int n_ages, int max_slots, int N, double cut, double* out, int* used,
                              void* stream) {
    PoolArgs a;
    PoolPlans pl;
    if (!plans_host_array) return VST_E_ARG;
    if (int rc = pool_args(records_host_array, weights_host, n_ages, max_slots, N, cut, out, used, a)) return rc;
    for (int k = 0; k < POOL_MAX_AGES; ++k) {
        pl.plan[k] = k < n_ages ? (const LabelPlan*)plans_host_array[k] : nullptr;
        if (k < n_ages && (!pl.plan[k] || ((uintptr_t)pl.plan[k] & 3))) return VST_E_ARG;
    }
    hipStream_t st = (hipStream_t)stream;
    vst_prof_scope prof(VST_KERNEL_CWCT_POOL, st);
    cwct_stats_pool_keyed_kernel<<<max_slots, POOL_THREADS, 0, st>>>(a, pl, n_ages, N, cut, out, used);
    VST_RETURN_IF_LAUNCH_FAILED();
    return VST_OK;
}
