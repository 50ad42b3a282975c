// Width-generic cWCT: every code width N = 1..256 that has no tuned kernel (cwct.hip covers N in {16, 32, 64, 128}).
//
// Reference: models/cWCT.py:111-262 (cholesky_dec, whitening, coloring, _transfer_seg, interpolation) works for any N; a
// RevResNet built with another hidden_dim (models/RevResNet.py:166-201) hands the cWCT a code of N = 2 * hidden_dim channels.
// Same records and arithmetic as the tuned fp32 calls, with N a runtime argument:
//   stats  : per-workgroup shifted fp32 sums (shift = the workgroup's first pixel), combined in fp64 (Chan et al.), the
//            record of cwct.hip (n, shift, sum, co-moment).  N <= 16: every thread accumulates the outer products of its own
//            pixels in registers (no LDS in the loop); N > 16: 64-pixel tiles staged in LDS, the N x N co-moment cut into
//            (16 RB)^2 channel-block pairs, one workgroup per (pixel range, block pair).
//   factor : one workgroup; fp32 Cholesky with LAPACK's failure rule and the cumulative jitter schedule, the mix, the solve
//            T Lc = mixL, t0 = mix_mean - T mean_c.  The matrices live in a global workspace (N = 256 does not fit the LDS).
//   apply  : y[:, p] = T x[:, p] + t0 in exact fp32 (or fp64 accumulation for the fp64 affine record); a tile of pixels is
//            staged in LDS before anything is written, so y may alias x.
// Not tuned: correctness first (DESIGN.md section 5 has what they are not tuned for).
#include "common.h"

#define CWCTN_MAX_N 256
#define CWCTN_MAX_STYLES 8         // = CWCT_MAX_STYLES of cwct.hip
#define CWCTN_MAX_TRIES 4096       // = CWCT_MAX_TRIES
#define CWCTN_FACTOR_THREADS 1024

static inline size_t cwctn_stride(int N) { return (size_t)N * N + 2 * N + 4; }    // = cwct_partial_stride of cwct.hip
__device__ __forceinline__ size_t cwctn_stride_d(int N) { return (size_t)N * N + 2 * N + 4; }

// pixels per workgroup and workgroup count of the statistics passes (the rule of cwct.hip's cwct_stats_groups)
static inline int cwctn_groups(long L, int* px_per_wg) {
    long per = 2048;
    while (per > 512 && L / per < 256) per >>= 1;
    long g = (L + per - 1) / per;
    if (g > 1024) { g = 1024; per = ((L + g - 1) / g + 63) / 64 * 64; g = (L + per - 1) / per; }
    *px_per_wg = (int)per;
    return (int)g;
}

// ================================================================================================
// statistics, N <= NP <= 16: registers only.  Thread t takes pixels p_begin + t, + 256, ...; per pixel the NP (zero-padded)
// shifted inputs and the NP (NP + 1) / 2 products of the upper triangle.  The workgroup's sums go through 64-lane shuffles
// and one LDS exchange at the end, in fp64: the record is fp32, and behind a shift that lies a few deviations off the mean
// q - a^2 / n cancels several-fold, so the roundings of an fp32 tree (about u in q) came out at 5 u in a variance.
// ================================================================================================
// a wave's sum of v, in fp64
__device__ __forceinline__ double cwctn_wave_sum(float x) {
    double v = x;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

template <int NP>
__global__ __launch_bounds__(256) void cwctn_stats_reg_kernel(const float* __restrict__ x, int N, long L,
                                                              const uint8_t* __restrict__ mask, int label,
                                                              float* __restrict__ partial, int px_per_wg) {
    constexpr int NQ = NP * (NP + 1) / 2, NV = NQ + NP + 1;
    __shared__ double red[4][NV];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long p_begin = (long)blockIdx.x * px_per_wg;
    const long p_end = p_begin + px_per_wg < L ? p_begin + px_per_wg : L;
    float sh[NP], s[NP], q[NQ], cnt = 0.f;
#pragma unroll
    for (int c = 0; c < NP; ++c) {
        sh[c] = c < N ? x[(size_t)c * L + p_begin] : 0.f;
        s[c] = 0.f;
    }
#pragma unroll
    for (int k = 0; k < NQ; ++k) q[k] = 0.f;
    for (long p = p_begin + tid; p < p_end; p += 256) {
        if (mask != nullptr && mask[p] != label) continue;
        float v[NP];
#pragma unroll
        for (int c = 0; c < NP; ++c) v[c] = c < N ? x[(size_t)c * L + p] - sh[c] : 0.f;
        cnt += 1.f;
#pragma unroll
        for (int c = 0; c < NP; ++c) s[c] += v[c];
        int k = 0;
#pragma unroll
        for (int i = 0; i < NP; ++i)
#pragma unroll
            for (int j = i; j < NP; ++j, ++k) q[k] = fmaf(v[i], v[j], q[k]);
    }
    // workgroup sums: {q, s, cnt}
#pragma unroll
    for (int k = 0; k < NQ; ++k) {
        const double v = cwctn_wave_sum(q[k]);
        if (lane == 0) red[wave][k] = v;
    }
#pragma unroll
    for (int c = 0; c < NP; ++c) {
        const double v = cwctn_wave_sum(s[c]);
        if (lane == 0) red[wave][NQ + c] = v;
    }
    {
        const double v = cwctn_wave_sum(cnt);
        if (lane == 0) red[wave][NQ + NP] = v;
    }
    __syncthreads();
    float* rec = partial + (size_t)blockIdx.x * cwctn_stride_d(N);
    for (int k = tid; k < NV; k += 256) {
        const float v = (float)((red[0][k] + red[1][k]) + (red[2][k] + red[3][k]));
        if (k < NQ) {
            int i = 0, r = k;                               // k -> (i, j), j >= i, row-major over the upper triangle
            while (r >= NP - i) { r -= NP - i; ++i; }
            const int j = i + r;
            if (i < N && j < N) {
                rec[4 + 2 * N + (size_t)i * N + j] = v;
                rec[4 + 2 * N + (size_t)j * N + i] = v;
            }
        } else if (k < NQ + NP) {
            const int c = k - NQ;
            if (c < N) { rec[4 + N + c] = v; rec[4 + c] = x[(size_t)c * L + p_begin]; }     // (= sh[c])
        } else {
            rec[0] = v;
        }
    }
}

// ================================================================================================
// statistics, N > 16: channel-block pairs.  TN = 16 RB channels per block, nb = ceil(N / TN) blocks, blockIdx.y = pair
// (bi <= bj).  A 64-pixel tile of both blocks is staged shifted (zeros for masked-out pixels and channels >= N) in LDS;
// thread (ti, tj) owns entries (ti + 16 a, tj + 16 b) of the pair's TN x TN co-moment block.  Diagonal pairs also write
// the shifts and sums of their channels, pair (0, 0) the count.  No chain of dependent fp32 additions runs over a whole
// workgroup: a tile's 64 pixels go into accumulators of their own, added to the running totals once per tile, and the row sums
// go 4 pixels, 4 steps, 4 steps per tile (one chain over a workgroup's 512 .. 2112 pixels sat at 4 .. 6.7 x the fp32
// restatement's error, a row-sum chain of 16 steps per tile still at 4.02; cwct.hip sums per tile for the same reason).
// ================================================================================================
template <int RB>
__global__ __launch_bounds__(256) void cwctn_stats_tile_kernel(const float* __restrict__ x, int N, long L,
                                                               const uint8_t* __restrict__ mask, int label,
                                                               float* __restrict__ partial, int px_per_wg) {
    constexpr int TN = 16 * RB, PT = 64, LD = PT + 4;
    __shared__ __attribute__((aligned(16))) float xa[TN * LD];
    __shared__ __attribute__((aligned(16))) float xb[TN * LD];
    __shared__ __attribute__((aligned(16))) float vflag[PT];
    __shared__ float sha[TN], shb[TN];
    const int tid = threadIdx.x, ti = tid >> 4, tj = tid & 15;
    const int nb = (N + TN - 1) / TN;
    int bi = 0, r = blockIdx.y;
    while (r >= nb - bi) { r -= nb - bi; ++bi; }
    const int bj = bi + r;
    const bool diag = bi == bj;
    const int ca0 = bi * TN, cb0 = bj * TN;
    const long p_begin = (long)blockIdx.x * px_per_wg;
    const long p_end = p_begin + px_per_wg < L ? p_begin + px_per_wg : L;
    for (int c = tid; c < TN; c += 256) {
        sha[c] = ca0 + c < N ? x[(size_t)(ca0 + c) * L + p_begin] : 0.f;
        shb[c] = cb0 + c < N ? x[(size_t)(cb0 + c) * L + p_begin] : 0.f;
    }
    const float* xbs = diag ? xa : xb;
    float q[RB][RB], asum[RB], cnt = 0.f;
#pragma unroll
    for (int a = 0; a < RB; ++a) {
        asum[a] = 0.f;
#pragma unroll
        for (int b = 0; b < RB; ++b) q[a][b] = 0.f;
    }
    for (long p0 = p_begin; p0 < p_end; p0 += PT) {
        __syncthreads();
        if (tid < PT) {
            const long p = p0 + tid;
            vflag[tid] = (p < p_end && (mask == nullptr || mask[p] == label)) ? 1.f : 0.f;
        }
        __syncthreads();
        for (int idx = tid; idx < TN * PT; idx += 256) {
            const int c = idx >> 6, pl = idx & 63;
            const long p = p0 + pl;
            const bool on = vflag[pl] != 0.f;
            xa[c * LD + pl] = on && ca0 + c < N ? x[(size_t)(ca0 + c) * L + p] - sha[c] : 0.f;
            if (!diag) xb[c * LD + pl] = on && cb0 + c < N ? x[(size_t)(cb0 + c) * L + p] - shb[c] : 0.f;
        }
        __syncthreads();
        float tq[RB][RB], ts[RB], gs[RB];
#pragma unroll
        for (int a = 0; a < RB; ++a) {
            ts[a] = gs[a] = 0.f;
#pragma unroll
            for (int b = 0; b < RB; ++b) tq[a][b] = 0.f;
        }
#pragma unroll 4
        for (int pl = 0; pl < PT; pl += 4) {
            float4 av[RB], bv[RB];
#pragma unroll
            for (int a = 0; a < RB; ++a) {
                av[a] = *(const float4*)&xa[(ti + 16 * a) * LD + pl];
                bv[a] = *(const float4*)&xbs[(tj + 16 * a) * LD + pl];
            }
            const float4 vf = *(const float4*)&vflag[pl];
            cnt += vf.x + vf.y + vf.z + vf.w;
            const bool last = (pl & 12) == 12;                // the 4th step of a group of 16 pixels
#pragma unroll
            for (int a = 0; a < RB; ++a) {
                gs[a] += (av[a].x + av[a].y) + (av[a].z + av[a].w);
                if (last) { ts[a] += gs[a]; gs[a] = 0.f; }
#pragma unroll
                for (int b = 0; b < RB; ++b) {
                    tq[a][b] = fmaf(av[a].x, bv[b].x, tq[a][b]);
                    tq[a][b] = fmaf(av[a].y, bv[b].y, tq[a][b]);
                    tq[a][b] = fmaf(av[a].z, bv[b].z, tq[a][b]);
                    tq[a][b] = fmaf(av[a].w, bv[b].w, tq[a][b]);
                }
            }
        }
#pragma unroll
        for (int a = 0; a < RB; ++a) {
            asum[a] += ts[a];
#pragma unroll
            for (int b = 0; b < RB; ++b) q[a][b] += tq[a][b];
        }
    }
    float* rec = partial + (size_t)blockIdx.x * cwctn_stride_d(N);
    if (diag) {
        if (bi == 0 && tid == 0) rec[0] = cnt;
        for (int c = tid; c < TN; c += 256)
            if (ca0 + c < N) rec[4 + ca0 + c] = sha[c];
    }
#pragma unroll
    for (int a = 0; a < RB; ++a) {
        const int i = ca0 + ti + 16 * a;
        if (diag && tj == 0 && i < N) rec[4 + N + i] = asum[a];
#pragma unroll
        for (int b = 0; b < RB; ++b) {
            const int j = cb0 + tj + 16 * b;
            if (i < N && j < N) {
                rec[4 + 2 * N + (size_t)i * N + j] = q[a][b];
                if (!diag) rec[4 + 2 * N + (size_t)j * N + i] = q[a][b];
            }
        }
    }
}

// Combine the per-workgroup records in fp64 (cwct.hip's cwct_stats_mean_kernel / cwct_stats_cov_kernel with N a bound, not a
// multiple of 16): 16 threads per output, each summing G/16 records, then an LDS reduction.
__global__ __launch_bounds__(256) void cwctn_stats_mean_kernel(const float* __restrict__ partial, int G, int N,
                                                               double* __restrict__ stats) {
    __shared__ double sacc[16][17], snt[16][17];
    const int cl = threadIdx.x & 15, gl = threadIdx.x >> 4;
    const int c = blockIdx.x * 16 + cl;
    const int cc = c < N ? c : N - 1;
    const size_t PS = cwctn_stride_d(N);
    double acc = 0.0, nt = 0.0;
#pragma unroll 4
    for (int g = gl; g < G; g += 16) {
        const float* rec = partial + (size_t)g * PS;
        const double n = rec[0];
        nt += n;
        acc += n * (double)rec[4 + cc] + (double)rec[4 + N + cc];
    }
    sacc[gl][cl] = acc; snt[gl][cl] = nt;
    __syncthreads();
    if (gl == 0 && c < N) {
        double a2 = 0.0, n2 = 0.0;
        for (int k = 0; k < 16; ++k) { a2 += sacc[k][cl]; n2 += snt[k][cl]; }
        stats[1 + c] = n2 > 0.0 ? a2 / n2 : 0.0;
        if (c == 0) stats[0] = n2;
    }
}

__global__ __launch_bounds__(256) void cwctn_stats_cov_kernel(const float* __restrict__ partial, int G, int N,
                                                              double* __restrict__ stats) {
    __shared__ double sm2[16][17];
    const int el = threadIdx.x & 15, gl = threadIdx.x >> 4;
    const int e = blockIdx.x * 16 + el;
    const int ee = e < N * N ? e : N * N - 1;
    const int i = ee / N, j = ee - i * N;
    const size_t PS = cwctn_stride_d(N);
    const double mu_i = stats[1 + i], mu_j = stats[1 + j];
    double m2 = 0.0;
#pragma unroll 4
    for (int g = gl; g < G; g += 16) {
        const float* rec = partial + (size_t)g * PS;
        const float nf = rec[0], aif = rec[4 + N + i], ajf = rec[4 + N + j], si = rec[4 + i], sj = rec[4 + j],
                    q = rec[4 + 2 * N + ee];
        const double n = nf, ai = aif, aj = ajf;
        const double rn = nf > 0.f ? 1.0 / n : 0.0;
        const double di = (double)si + ai * rn - mu_i;
        const double dj = (double)sj + aj * rn - mu_j;
        m2 += nf > 0.f ? (double)q - ai * aj * rn + n * di * dj : 0.0;
    }
    sm2[gl][el] = m2;
    __syncthreads();
    if (gl == 0 && e < N * N) {
        double t = 0.0;
        for (int k = 0; k < 16; ++k) t += sm2[k][el];
        stats[1 + N + e] = t / (stats[0] - 1.0);
    }
}

// ================================================================================================
// factor (fp32), one workgroup of 1024 threads, matrices in a global workspace (N * N floats) and in `affine` itself
// ================================================================================================
struct FactorNArgs {
    const double* content;
    const double* styles[CWCTN_MAX_STYLES];
    float alphas[CWCTN_MAX_STYLES];
    int n_styles;
    float alpha_c, eps;
    int N;
    float* affine;
    int* info;
    float* ws;
};

// lower Cholesky factor of the covariance in `stats` into A (row-major N x N, upper triangle zeroed), fp32 with LAPACK's failure
// rule (pivot <= 0 or NaN) and the reference's cumulative jitter (eps, 2 eps, ... each rounded to fp32 and added in fp32, as
// cwct.hip's fac_load); a prefactored record (stats[0] < 0) holds the factor.  Returns the retries.  Right-looking, two barriers
// per column: scale the column below the pivot, then the rank-1 update of the trailing lower triangle (and the pivot itself).
__device__ int cwctn_chol(float* A, const double* stats, int N, float eps, int min_tries) {
    const int tid = threadIdx.x, NT = blockDim.x;
    const double* cov = stats + 1 + N;
    if (stats[0] < 0.0) {
        for (int e = tid; e < N * N; e += NT) A[e] = (float)cov[e];
        __syncthreads();
        return 0;
    }
    int tries = min_tries < 0 ? 0 : (min_tries > CWCTN_MAX_TRIES ? CWCTN_MAX_TRIES : min_tries);
    while (true) {
        for (int e = tid; e < N * N; e += NT) {
            float v = (float)cov[e];
            if (e / N == e % N)
                for (int t = 1; t <= tries; ++t) v = v + (float)((double)t * (double)eps);
            A[e] = v;
        }
        __syncthreads();
        bool failed = false;
        for (int j = 0; j < N; ++j) {
            const float d = A[j * N + j];                  // every thread reads the same word: a uniform decision
            if (!(d > 0.f)) { failed = true; break; }
            const float piv = sqrtf(d);
            const float rpiv = 1.0f / piv;                  // LAPACK's potf2 scales the column by 1/ajj
            for (int i = j + 1 + tid; i < N; i += NT) A[i * N + j] *= rpiv;
            __syncthreads();                                // (every thread has read d before anyone writes the pivot)
            if (tid == 0) A[j * N + j] = piv;
            const int m = N - j - 1;
            for (int e = tid; e < m * m; e += NT) {
                const int i = j + 1 + e / m, k = j + 1 + e % m;
                if (k <= i) A[i * N + k] -= A[i * N + j] * A[k * N + j];
            }
            __syncthreads();
        }
        __syncthreads();                                    // (a failed pass: every thread is done reading A)
        if (!failed || tries >= CWCTN_MAX_TRIES) break;
        ++tries;
    }
    for (int e = tid; e < N * N; e += NT)
        if (e % N > e / N) A[e] = 0.f;
    __syncthreads();
    return tries;
}

__global__ __launch_bounds__(CWCTN_FACTOR_THREADS) void cwctn_factor_kernel(const FactorNArgs a) {
    const int N = a.N, tid = threadIdx.x, NT = blockDim.x;
    float* A = a.ws;           // Cholesky factors, one at a time; Lc at the end
    float* M = a.affine;       // mixL, then T (the solve runs in place)
    for (int e = tid; e < N * N; e += NT) M[e] = 0.f;
    for (int s = 0; s < a.n_styles; ++s) {
        const int min_tries = a.info[2 + s];
        __syncthreads();
        const int tries = cwctn_chol(A, a.styles[s], N, a.eps, min_tries);
        if (tid == 0) a.info[2 + s] = tries;
        const float al = a.alphas[s];
        for (int e = tid; e < N * N; e += NT) M[e] += A[e] * al;
        __syncthreads();
    }
    const int cmin = a.info[0];
    __syncthreads();
    const int ctries = cwctn_chol(A, a.content, N, a.eps, cmin);
    if (tid == 0) { a.info[0] = ctries; a.info[1] = ctries >= CWCTN_MAX_TRIES; }
    const float ac = a.alpha_c;
    if (ac != 0.f)
        for (int e = tid; e < N * N; e += NT) M[e] = M[e] * (1.f - ac) + A[e] * ac;
    __syncthreads();
    // T Lc = mixL, last column first (cwct.hip's solve): T[:, j] = M[:, j] / Lc[j][j], then M[i][k] -= T[i][j] Lc[j][k], k < j.
    // Rows i < j of a lower-triangular M hold zeros in column j and are skipped.
    for (int j = N - 1; j >= 0; --j) {
        const float rljj = 1.0f / A[j * N + j];
        for (int i = j + tid; i < N; i += NT) M[i * N + j] *= rljj;
        __syncthreads();
        const int rows = N - j;
        for (int e = tid; e < rows * j; e += NT) {
            const int i = j + e / j, k = e % j;
            M[i * N + k] -= M[i * N + j] * A[j * N + k];
        }
        __syncthreads();
    }
    // t0 = mix_mean - T mean_c
    if (tid < N) {
        double mm = 0.0;
        for (int s = 0; s < a.n_styles; ++s) mm += (double)(float)a.styles[s][1 + tid] * (double)a.alphas[s];
        if (ac != 0.f) mm = mm * (double)(1.f - ac) + (double)(float)a.content[1 + tid] * (double)ac;
        double part = 0.0;
        for (int k = 0; k <= tid; ++k) part += (double)M[tid * N + k] * a.content[1 + k];
        a.affine[N * N + tid] = (float)(mm - part);
    }
}

// stats {n, mean, cov} -> prefactored record {-(n+1), mean, L} (out may alias stats)
__global__ __launch_bounds__(CWCTN_FACTOR_THREADS) void cwctn_prefactor_kernel(const double* stats, int N, float eps, double* out,
                                                                               int* info, float* ws) {
    const int tid = threadIdx.x, NT = blockDim.x;
    const int tries = cwctn_chol(ws, stats, N, eps, 0);
    const double n = stats[0];
    const double mean = tid < N ? stats[1 + tid] : 0.0;
    __syncthreads();                                        // every read of stats is done
    if (tid == 0) { out[0] = n < 0.0 ? n : -(n + 1.0); info[0] = tries; }
    if (tid < N) out[1 + tid] = mean;
    for (int e = tid; e < N * N; e += NT) out[1 + N + e] = (double)ws[e];
}

// ================================================================================================
// apply: y[:, p] = T x[:, p] + t0.  A workgroup stages the N (padded to NP = 16k, zero rows) inputs of its 64 PG pixels in LDS,
// then each wave takes (16-row output block, 64-pixel group) items: lane = pixel, 16 accumulators, T / t0 read at uniform
// addresses (the scalar path).  Accumulation as cwct.hip's cwct_apply_kernel: acc = t0[i], then fma over j ascending (fp32 for
// a float record; a double record, the fp64 route, accumulates in fp64 and rounds once).  Reads all precede the barrier and
// workgroups own disjoint pixels: y may alias x.  With a mask only pixels whose label matches are written.
// ================================================================================================
template <typename TA>
__device__ __forceinline__ TA cwctn_fma(TA t, float xv, TA acc) { return fma(t, (TA)xv, acc); }
template <>
__device__ __forceinline__ float cwctn_fma<float>(float t, float xv, float acc) { return fmaf(t, xv, acc); }

template <typename TA, int PG>
__global__ __launch_bounds__(256) void cwctn_apply_kernel(const float* x, float* y, int N, long L, const TA* __restrict__ affine,
                                                          const uint8_t* __restrict__ mask, int label) {
    constexpr int P = 64 * PG;
    extern __shared__ __attribute__((aligned(16))) float xs[];     // [NP][P]
    const int NP = (N + 15) & ~15;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long p0 = (long)blockIdx.x * P;
    for (int e = tid; e < NP * P; e += 256) {
        const int c = e / P, k = e - c * P;
        const long p = p0 + k;
        xs[e] = (c < N && p < L) ? x[(size_t)c * L + p] : 0.f;
    }
    __syncthreads();
    const TA* t0 = affine + (size_t)N * N;
    const int items = (NP / 16) * PG;
    for (int it = wave; it < items; it += 4) {
        const int rb = it / PG, pg = it - rb * PG;
        const int k = pg * 64 + lane;
        const long p = p0 + k;
        const bool on = p < L && (mask == nullptr || mask[p] == label);
        TA acc[16];
#pragma unroll
        for (int o = 0; o < 16; ++o) acc[o] = rb * 16 + o < N ? t0[rb * 16 + o] : (TA)0;
        for (int j0 = 0; j0 < NP; j0 += 16) {
            float xv[16];
#pragma unroll
            for (int jj = 0; jj < 16; ++jj) xv[jj] = xs[(j0 + jj) * P + k];
            if (j0 + 16 <= N) {
#pragma unroll
                for (int o = 0; o < 16; ++o) {
                    const int i = rb * 16 + o;
                    if (i < N) {
                        const TA* row = affine + (size_t)i * N + j0;
#pragma unroll
                        for (int jj = 0; jj < 16; ++jj) acc[o] = cwctn_fma<TA>(row[jj], xv[jj], acc[o]);
                    }
                }
            } else {                                        // the last, partial column block
#pragma unroll
                for (int o = 0; o < 16; ++o) {
                    const int i = rb * 16 + o;
                    if (i < N) {
                        const TA* row = affine + (size_t)i * N + j0;
#pragma unroll
                        for (int jj = 0; jj < 16; ++jj)
                            if (j0 + jj < N) acc[o] = cwctn_fma<TA>(row[jj], xv[jj], acc[o]);
                    }
                }
            }
        }
        if (on) {
#pragma unroll
            for (int o = 0; o < 16; ++o)
                if (rb * 16 + o < N) y[(size_t)(rb * 16 + o) * L + p] = (float)acc[o];
        }
    }
}

template <typename TA>
static int cwctn_apply_launch(const float* x, float* y, int N, long L, const TA* affine, const uint8_t* mask, int label,
                              hipStream_t st) {
    const int NP = (N + 15) & ~15;
    // pixels per workgroup: 256 for N <= 32, 128 for N <= 64, 64 above (at most 64 KiB of staged inputs)
    const int PG = NP <= 32 ? 4 : (NP <= 64 ? 2 : 1);
    const size_t lds = (size_t)NP * 64 * PG * sizeof(float);
    const unsigned grid = (unsigned)((L + 64 * PG - 1) / (64 * PG));
    static std::atomic<unsigned> attr_done{0};
    switch (PG) {
        case 4: cwctn_apply_kernel<TA, 4><<<grid, 256, lds, st>>>(x, y, N, L, affine, mask, label); break;
        case 2: cwctn_apply_kernel<TA, 2><<<grid, 256, lds, st>>>(x, y, N, L, affine, mask, label); break;
        default:
            if (int rc = vst_ensure_dynamic_lds((const void*)cwctn_apply_kernel<TA, 1>, 65536, &attr_done)) return rc;
            cwctn_apply_kernel<TA, 1><<<grid, 256, lds, st>>>(x, y, N, L, affine, mask, label);
            break;
    }
    VST_RETURN_IF_LAUNCH_FAILED();
    return VST_OK;
}

extern "C" {

size_t vst_cwct_stats_n_workspace_bytes(int N, long L) {
    if (N < 1 || N > CWCTN_MAX_N || L <= 0) return 0;
    int per;
    const int g = cwctn_groups(L, &per);
    return (size_t)g * cwctn_stride(N) * sizeof(float);
}

int vst_cwct_stats_n(const float* x, int N, long L, const uint8_t* mask, int label, double* stats, void* workspace,
                     size_t workspace_bytes, void* stream) {
    if (!x || !stats || L <= 0) return VST_E_ARG;
    if (N < 1 || N > CWCTN_MAX_N) return VST_E_SHAPE;
    if (!workspace || workspace_bytes < vst_cwct_stats_n_workspace_bytes(N, L)) return VST_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    int per;
    const int G = cwctn_groups(L, &per);
    float* partial = (float*)workspace;
    vst_prof_scope prof(VST_KERNEL_CWCT_STATS, st);
    if (N <= 4) {
        cwctn_stats_reg_kernel<4><<<G, 256, 0, st>>>(x, N, L, mask, label, partial, per);
    } else if (N <= 8) {
        cwctn_stats_reg_kernel<8><<<G, 256, 0, st>>>(x, N, L, mask, label, partial, per);
    } else if (N <= 16) {
        cwctn_stats_reg_kernel<16><<<G, 256, 0, st>>>(x, N, L, mask, label, partial, per);
    } else if (N <= 32) {
        cwctn_stats_tile_kernel<2><<<dim3(G, 1), 256, 0, st>>>(x, N, L, mask, label, partial, per);
    } else {
        const int nb = (N + 63) / 64;
        cwctn_stats_tile_kernel<4><<<dim3(G, nb * (nb + 1) / 2), 256, 0, st>>>(x, N, L, mask, label, partial, per);
    }
    VST_RETURN_IF_LAUNCH_FAILED();
    cwctn_stats_mean_kernel<<<(N + 15) / 16, 256, 0, st>>>(partial, G, N, stats);
    VST_RETURN_IF_LAUNCH_FAILED();
    cwctn_stats_cov_kernel<<<(N * N + 15) / 16, 256, 0, st>>>(partial, G, N, stats);
    VST_RETURN_IF_LAUNCH_FAILED();
    return VST_OK;
}

size_t vst_cwct_factor_n_workspace_bytes(int N) {
    return N >= 1 && N <= CWCTN_MAX_N ? (size_t)N * N * sizeof(float) : 0;
}

int vst_cwct_factor_n(const double* content_stats, const double* const* style_stats_host_array, const float* alphas_host,
                      int n_styles, float alpha_c, float eps, int N, float* affine, int* info, void* workspace,
                      size_t workspace_bytes, void* stream) {
    if (!content_stats || !style_stats_host_array || !alphas_host || !affine || !info) return VST_E_ARG;
    if (n_styles < 1 || n_styles > CWCTN_MAX_STYLES) return VST_E_ARG;
    for (int i = 0; i < n_styles; ++i)
        if (!style_stats_host_array[i]) return VST_E_ARG;
    if (N < 1 || N > CWCTN_MAX_N) return VST_E_SHAPE;
    if (!workspace || workspace_bytes < vst_cwct_factor_n_workspace_bytes(N)) return VST_E_WORKSPACE;
    FactorNArgs a{};
    a.content = content_stats;
    for (int i = 0; i < n_styles; ++i) {
        a.styles[i] = style_stats_host_array[i];
        a.alphas[i] = alphas_host[i];
    }
    a.n_styles = n_styles; a.alpha_c = alpha_c; a.eps = eps; a.N = N; a.affine = affine; a.info = info;
    a.ws = (float*)workspace;
    hipStream_t st = (hipStream_t)stream;
    vst_prof_scope prof(VST_KERNEL_CWCT_FACTOR, st);
    cwctn_factor_kernel<<<1, CWCTN_FACTOR_THREADS, 0, st>>>(a);
    VST_RETURN_IF_LAUNCH_FAILED();
    return VST_OK;
}

int vst_cwct_prefactor_n(const double* stats, int N, float eps, double* out, int* info, void* workspace, size_t workspace_bytes,
                         void* stream) {
    if (!stats || !out || !info) return VST_E_ARG;
    if (N < 1 || N > CWCTN_MAX_N) return VST_E_SHAPE;
    if (!workspace || workspace_bytes < vst_cwct_factor_n_workspace_bytes(N)) return VST_E_WORKSPACE;
    cwctn_prefactor_kernel<<<1, CWCTN_FACTOR_THREADS, 0, (hipStream_t)stream>>>(stats, N, eps, out, info, (float*)workspace);
    VST_RETURN_IF_LAUNCH_FAILED();
    return VST_OK;
}

int vst_cwct_apply_n(const float* x, float* y, int N, long L, const float* affine, const uint8_t* mask, int label, void* stream) {
    if (!x || !y || !affine || L <= 0) return VST_E_ARG;
    if (N < 1 || N > CWCTN_MAX_N) return VST_E_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    vst_prof_scope prof(VST_KERNEL_CWCT_APPLY, st);
    return cwctn_apply_launch<float>(x, y, N, L, affine, mask, label, st);
}

int vst_cwct_apply_n_f64(const float* x, float* y, int N, long L, const double* affine, const uint8_t* mask, int label,
                         void* stream) {
    if (!x || !y || !affine || L <= 0) return VST_E_ARG;
    if (N < 1 || N > CWCTN_MAX_N) return VST_E_SHAPE;
    return cwctn_apply_launch<double>(x, y, N, L, affine, mask, label, (hipStream_t)stream);
}

}  // extern "C"
