// Optical flow (vstnet.h, "Optical flow"): a coarse-to-fine, warping Lucas-Kanade estimator on a pair of uint8
// frames, the forward-backward consistency mask, and the temporal L1 restricted to that mask.
//
// Every step of the estimator is continuous in its inputs (no median, no argmin, no threshold on a determinant) and all of its
// arithmetic is fp64 without contraction, so the device can be held to a numpy statement of the same formulas (tests/flow_ref.py)
// to within the last rounding to fp32.  Pyramids and the field stay fp64 in the workspace.  Nothing here uses an atomic: every
// output element is written by one thread from sums taken in a fixed order, so two runs give the same bits.
//
// The iteration is the hot kernel (lk_iter_kernel): a workgroup owns a 32 x 32 tile, gathers the bilinear samples of the tile plus
// a halo of `radius`, keeps Rx e and Ry e in LDS, forms the window sums from LDS separably (rows, then columns), solves the 2 x 2
// system, clamps and writes d.  A row of the tile is 32 doubles = one 256-byte bank row, and a 32-lane half of a wave reads 32
// consecutive doubles of one LDS row in both passes: the 8-byte reads are free of bank conflicts whatever the halo's row stride.
// LDS: 2 x 46 x 46 + 2 x 46 x 32 doubles = 57408 bytes at the largest radius (7), two workgroups per CU.
#include "common.h"
#include <math.h>

#pragma clang fp contract(off)

namespace {

constexpr int TW = 32, TH = 32;                  // the tile of the LDS kernels
constexpr int RMAX = VST_FLOW_MAX_RADIUS;
constexpr int SIDE = TW + 2 * RMAX;              // the tile with its largest halo
constexpr int THREADS = 256;
constexpr int PER_THREAD = TW * TH / THREADS;    // outputs of one thread
constexpr int MAX_LEVELS = VST_FLOW_MAX_LEVELS;

// ---- the pyramid's geometry and the workspace.  Per level: R, S, dx, dy.  Once, at the frame's size: the update before its
// smoothing (tx, ty), the gradients (Rx, Ry) and the tensor (A11, A12, A22) of the level being worked on.
struct Pyramid {
    int n;
    int h[MAX_LEVELS], w[MAX_LEVELS];
    size_t at[MAX_LEVELS];                       // offset of the level, in pixels, inside a per-level plane
    size_t pixels;                               // all levels
};

Pyramid make_pyramid(int h, int w, int levels) {
    Pyramid p;
    p.n = 1, p.h[0] = h, p.w[0] = w, p.at[0] = 0, p.pixels = (size_t)h * w;
    while (p.n < levels) {
        const int nh = (p.h[p.n - 1] + 1) / 2, nw = (p.w[p.n - 1] + 1) / 2;
        if ((nh < nw ? nh : nw) < 8) break;
        p.h[p.n] = nh, p.w[p.n] = nw, p.at[p.n] = p.pixels, p.pixels += (size_t)nh * nw;
        ++p.n;
    }
    return p;
}

constexpr int PLANES_PER_LEVEL = 4, PLANES_ONCE = 7;

size_t workspace_doubles(const Pyramid& p) { return PLANES_PER_LEVEL * p.pixels + PLANES_ONCE * (size_t)p.h[0] * p.w[0]; }

__device__ __forceinline__ int clampi(int v, int n) { return v < 0 ? 0 : (v > n - 1 ? n - 1 : v); }

// bilinear(A; y, x) with the coordinates clamped to the frame; fmax / fmin return the other operand for a NaN, so the indices
// stay inside the plane whatever the coordinate is
__device__ __forceinline__ double bilinear(const double* __restrict__ A, int h, int w, double y, double x) {
    x = fmin(fmax(x, 0.0), (double)(w - 1));
    y = fmin(fmax(y, 0.0), (double)(h - 1));
    const int x0 = clampi((int)floor(x), w), y0 = clampi((int)floor(y), h);
    const int x1 = x0 + 1 > w - 1 ? w - 1 : x0 + 1, y1 = y0 + 1 > h - 1 ? h - 1 : y0 + 1;
    const double fx = x - (double)x0, fy = y - (double)y0;
    const double* r0 = A + (size_t)y0 * w;
    const double* r1 = A + (size_t)y1 * w;
    const double top = (1.0 - fx) * r0[x0] + fx * r0[x1];
    const double bot = (1.0 - fx) * r1[x0] + fx * r1[x1];
    return (1.0 - fy) * top + fy * bot;
}

// the weight of a sample at coordinate c of an axis of n pixels: 1 inside, falling to 0 one pixel outside
__device__ __forceinline__ double inside_weight(double c, int n) {
    const double o = fmax(fmax(-c, c - (double)(n - 1)), 0.0);
    return fmin(fmax(1.0 - o, 0.0), 1.0);
}

// ---- grey level 0 of both frames: blockIdx.y = 0: ref, 1: src
__global__ __launch_bounds__(256) void grey_kernel(const uint8_t* __restrict__ ref, const uint8_t* __restrict__ src,
                                                   double* __restrict__ R, double* __restrict__ S, size_t hw) {
    const size_t at = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (at >= hw) return;
    const uint8_t* p = (blockIdx.y ? src : ref) + at * 3;
    const double g = (0.299 * (double)p[0] + 0.587 * (double)p[1] + 0.114 * (double)p[2]) / 255.0;
    (blockIdx.y ? S : R)[at] = g;
}

__constant__ double BINOMIAL[5] = {0.0625, 0.25, 0.375, 0.25, 0.0625};

__device__ __forceinline__ double binomial5(double a0, double a1, double a2, double a3, double a4) {
    return 0.0625 * a0 + 0.25 * a1 + 0.375 * a2 + 0.25 * a3 + 0.0625 * a4;
}

// ---- one level down: pixel (2y, 2x) of the binomial-filtered level (rows first, then columns), edges replicated
__global__ __launch_bounds__(256) void down_kernel(const double* __restrict__ R, const double* __restrict__ S,
                                                   double* __restrict__ Rn, double* __restrict__ Sn, int h, int w, int nh, int nw) {
    const size_t at = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (at >= (size_t)nh * nw) return;
    const double* A = blockIdx.y ? S : R;
    const int y = (int)(at / nw), x = (int)(at % nw);
    double row[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const double* a = A + (size_t)clampi(2 * y - 2 + j, h) * w;
        row[j] = binomial5(a[clampi(2 * x - 2, w)], a[clampi(2 * x - 1, w)], a[clampi(2 * x, w)], a[clampi(2 * x + 1, w)],
                           a[clampi(2 * x + 2, w)]);
    }
    (blockIdx.y ? Sn : Rn)[at] = binomial5(row[0], row[1], row[2], row[3], row[4]);
}

// ---- the field one level up: d_l(y, x) = 2 bilinear(d_{l+1}; y / 2, x / 2); blockIdx.y: component
__global__ __launch_bounds__(256) void up_kernel(const double* __restrict__ cx, const double* __restrict__ cy,
                                                 double* __restrict__ dx, double* __restrict__ dy, int h, int w, int ch, int cw) {
    const size_t at = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (at >= (size_t)h * w) return;
    const int y = (int)(at / w), x = (int)(at % w);
    (blockIdx.y ? dy : dx)[at] = 2.0 * bilinear(blockIdx.y ? cy : cx, ch, cw, 0.5 * (double)y, 0.5 * (double)x);
}

// ---- the separable window passes of the LDS kernels.  a, b: [TH + 2r][TW + 2r] values at the tile's pixels and its halo, window
// coordinates clamped to the frame by whoever filled them.  rows(): ha, hb [TH + 2r][TW] = the sum over the 2r + 1 columns of
// f(a, b); column(): the sum over the 2r + 1 rows of one of them.  wt: the taps' weights, or nullptr for ones.
template <typename F>
__device__ __forceinline__ void rows(const double* a, const double* b, double* ha, double* hb, int r, const double* wt, F f) {
    const int side_w = TW + 2 * r, n = (TH + 2 * r) * TW;
    for (int idx = threadIdx.x; idx < n; idx += THREADS) {
        const int j = idx / TW, i = idx % TW;
        const double* pa = a + j * side_w + i;
        const double* pb = b + j * side_w + i;
        double s1 = 0.0, s2 = 0.0;
        for (int k = 0; k <= 2 * r; ++k) {
            double p1, p2;
            f(pa[k], pb[k], p1, p2);
            const double wk = wt ? wt[k] : 1.0;
            s1 += wk * p1, s2 += wk * p2;
        }
        ha[idx] = s1, hb[idx] = s2;
    }
}

__device__ __forceinline__ double column(const double* hx, int y, int x, int r, const double* wt) {
    double s = 0.0;
    for (int k = 0; k <= 2 * r; ++k) s += (wt ? wt[k] : 1.0) * hx[(y + k) * TW + x];
    return s;
}

struct LdsTile {
    double a[SIDE * SIDE], b[SIDE * SIDE], ha[SIDE * TW], hb[SIDE * TW];
};

// ---- gradients and structure tensor of one level
__global__ __launch_bounds__(THREADS) void tensor_kernel(const double* __restrict__ R, double* __restrict__ Rx,
                                                         double* __restrict__ Ry, double* __restrict__ A11,
                                                         double* __restrict__ A12, double* __restrict__ A22, int h, int w, int r,
                                                         double lambda) {
    __shared__ LdsTile t;
    const int tx0 = blockIdx.x * TW, ty0 = blockIdx.y * TH, side_w = TW + 2 * r, side_h = TH + 2 * r;
    for (int idx = threadIdx.x; idx < side_h * side_w; idx += THREADS) {
        const int y = clampi(ty0 - r + idx / side_w, h), x = clampi(tx0 - r + idx % side_w, w);
        const double* row = R + (size_t)y * w;
        t.a[idx] = (row[clampi(x + 1, w)] - row[clampi(x - 1, w)]) / 2.0;
        t.b[idx] = (R[(size_t)clampi(y + 1, h) * w + x] - R[(size_t)clampi(y - 1, h) * w + x]) / 2.0;
    }
    __syncthreads();
    rows(t.a, t.b, t.ha, t.hb, r, nullptr, [](double gx, double gy, double& p1, double& p2) { p1 = gx * gx, p2 = gy * gy; });
    __syncthreads();
    double s11[PER_THREAD], s22[PER_THREAD];
#pragma unroll
    for (int k = 0; k < PER_THREAD; ++k) {
        const int idx = threadIdx.x + k * THREADS, y = idx / TW, x = idx % TW;
        s11[k] = column(t.ha, y, x, r, nullptr), s22[k] = column(t.hb, y, x, r, nullptr);
    }
    __syncthreads();
    rows(t.a, t.b, t.ha, t.hb, r, nullptr, [](double gx, double gy, double& p1, double& p2) { p1 = gx * gy, p2 = 0.0; });
    __syncthreads();
#pragma unroll
    for (int k = 0; k < PER_THREAD; ++k) {
        const int idx = threadIdx.x + k * THREADS, y = idx / TW, x = idx % TW;
        if (ty0 + y >= h || tx0 + x >= w) continue;
        const size_t at = (size_t)(ty0 + y) * w + tx0 + x;
        const int mid = (y + r) * side_w + x + r;
        Rx[at] = t.a[mid], Ry[at] = t.b[mid];
        A11[at] = s11[k] + lambda, A22[at] = s22[k] + lambda;
        A12[at] = column(t.ha, y, x, r, nullptr);
    }
}

// ---- one iteration: d + delta into (ox, oy), before its smoothing
__global__ __launch_bounds__(THREADS) void lk_iter_kernel(const double* __restrict__ R, const double* __restrict__ S,
                                                          const double* __restrict__ Rx, const double* __restrict__ Ry,
                                                          const double* __restrict__ A11, const double* __restrict__ A12,
                                                          const double* __restrict__ A22, const double* __restrict__ dx,
                                                          const double* __restrict__ dy, double* __restrict__ ox,
                                                          double* __restrict__ oy, int h, int w, int r) {
    __shared__ LdsTile t;
    const int tx0 = blockIdx.x * TW, ty0 = blockIdx.y * TH, side_w = TW + 2 * r, side_h = TH + 2 * r;
    for (int idx = threadIdx.x; idx < side_h * side_w; idx += THREADS) {
        const int y = clampi(ty0 - r + idx / side_w, h), x = clampi(tx0 - r + idx % side_w, w);
        const size_t at = (size_t)y * w + x;
        const double sx = (double)x + dx[at], sy = (double)y + dy[at];
        const double e = (bilinear(S, h, w, sy, sx) - R[at]) * inside_weight(sy, h) * inside_weight(sx, w);
        t.a[idx] = Rx[at] * e, t.b[idx] = Ry[at] * e;
    }
    __syncthreads();
    rows(t.a, t.b, t.ha, t.hb, r, nullptr, [](double va, double vb, double& p1, double& p2) { p1 = va, p2 = vb; });
    __syncthreads();
#pragma unroll
    for (int k = 0; k < PER_THREAD; ++k) {
        const int idx = threadIdx.x + k * THREADS, y = idx / TW, x = idx % TW;
        if (ty0 + y >= h || tx0 + x >= w) continue;
        const size_t at = (size_t)(ty0 + y) * w + tx0 + x;
        const double b1 = column(t.ha, y, x, r, nullptr), b2 = column(t.hb, y, x, r, nullptr);
        const double a11 = A11[at], a12 = A12[at], a22 = A22[at];
        const double det = a11 * a22 - a12 * a12;
        double ux = -((a22 * b1 - a12 * b2) / det), uy = -((a11 * b2 - a12 * b1) / det);
        ux = fmin(fmax(ux, -1.0), 1.0), uy = fmin(fmax(uy, -1.0), 1.0);
        ox[at] = dx[at] + ux, oy[at] = dy[at] + uy;
    }
}

// ---- d = binomial5(t) per component; the last one of level 0 also leaves flow = -d in fp32
__global__ __launch_bounds__(THREADS) void smooth_kernel(const double* __restrict__ tx, const double* __restrict__ ty,
                                                         double* __restrict__ dx, double* __restrict__ dy,
                                                         float* __restrict__ flow_or_null, int h, int w) {
    __shared__ double a[(TH + 4) * (TW + 4)], b[(TH + 4) * (TW + 4)], ha[(TH + 4) * TW], hb[(TH + 4) * TW];
    const double* wt = BINOMIAL;
    constexpr int r = 2, side_w = TW + 2 * r, side_h = TH + 2 * r;
    const int tx0 = blockIdx.x * TW, ty0 = blockIdx.y * TH;
    for (int idx = threadIdx.x; idx < side_h * side_w; idx += THREADS) {
        const int y = clampi(ty0 - r + idx / side_w, h), x = clampi(tx0 - r + idx % side_w, w);
        const size_t at = (size_t)y * w + x;
        a[idx] = tx[at], b[idx] = ty[at];
    }
    __syncthreads();
    rows(a, b, ha, hb, r, wt, [](double va, double vb, double& p1, double& p2) { p1 = va, p2 = vb; });
    __syncthreads();
#pragma unroll
    for (int k = 0; k < PER_THREAD; ++k) {
        const int idx = threadIdx.x + k * THREADS, y = idx / TW, x = idx % TW;
        if (ty0 + y >= h || tx0 + x >= w) continue;
        const size_t at = (size_t)(ty0 + y) * w + tx0 + x;
        const double sx = column(ha, y, x, r, wt), sy = column(hb, y, x, r, wt);
        dx[at] = sx, dy[at] = sy;
        if (flow_or_null) flow_or_null[at] = (float)(-sx), flow_or_null[(size_t)h * w + at] = (float)(-sy);
    }
}

// ---- forward-backward consistency (Sundaram, Brox and Keutzer), fp64
__global__ __launch_bounds__(256) void consistency_kernel(const float* __restrict__ fwd, const float* __restrict__ bwd,
                                                          uint8_t* __restrict__ valid, int h, int w) {
    const size_t hw = (size_t)h * w;
    const size_t at = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (at >= hw) return;
    const int y = (int)(at / w), x = (int)(at % w);
    const double fx = (double)fwd[at], fy = (double)fwd[hw + at];
    const double qx = (double)x - fx, qy = (double)y - fy;
    const bool inside = qx >= 0.0 && qx <= (double)(w - 1) && qy >= 0.0 && qy <= (double)(h - 1);
    // bilinear() of a float plane, in fp64
    const double cx = fmin(fmax(qx, 0.0), (double)(w - 1)), cy = fmin(fmax(qy, 0.0), (double)(h - 1));
    const int x0 = clampi((int)floor(cx), w), y0 = clampi((int)floor(cy), h);
    const int x1 = x0 + 1 > w - 1 ? w - 1 : x0 + 1, y1 = y0 + 1 > h - 1 ? h - 1 : y0 + 1;
    const double ax = cx - (double)x0, ay = cy - (double)y0;
    double bv[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const float* r0 = bwd + c * hw + (size_t)y0 * w;
        const float* r1 = bwd + c * hw + (size_t)y1 * w;
        const double top = (1.0 - ax) * (double)r0[x0] + ax * (double)r0[x1];
        const double bot = (1.0 - ax) * (double)r1[x0] + ax * (double)r1[x1];
        bv[c] = (1.0 - ay) * top + ay * bot;
    }
    const double sx = fx + bv[0], sy = fy + bv[1];
    const double lhs = sx * sx + sy * sy;
    const double rhs = 0.01 * ((fx * fx + fy * fy) + (bv[0] * bv[0] + bv[1] * bv[1])) + 0.5;
    valid[at] = (inside && lhs <= rhs) ? 1 : 0;
}

// ---- the temporal L1 over the valid pixels: temporal.hip's two launches with a count beside the three sums.  A workgroup sums
// 2048 pixels: each sum is below 2^20 and the count below 2^12, so the count rides in the high half of the first partial and the
// workspace is the unmasked call's.
constexpr int L1_PER_THREAD = 8, L1_BLOCK_PIXELS = 256 * L1_PER_THREAD;

__device__ __forceinline__ int warp_index(int p, float flo, int n) {      // temporal.hip's, to the letter
    const float v = (float)p - flo;
    const float d = (float)(n > 1 ? n - 1 : 1);
    float t = 2.0f * v;
    t = t / d;
    t = t - 1.0f;
    float i = t + 1.0f;
    i = i * (float)n;
    i = i - 1.0f;
    i = i / 2.0f;
    i = fminf(fmaxf(i, 0.0f), (float)(n - 1));
    const int r = (int)rintf(i);
    return r < 0 ? 0 : (r > n - 1 ? n - 1 : r);
}

template <typename Acc>
__device__ __forceinline__ void block_tree4(Acc* red, const Acc (&s)[4], int tid) {
#pragma unroll
    for (int c = 0; c < 4; ++c) red[c * 256 + tid] = s[c];
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if (tid < k) {
#pragma unroll
            for (int c = 0; c < 4; ++c) red[c * 256 + tid] += red[c * 256 + tid + k];
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void l1_masked_kernel(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b,
                                                        const float* __restrict__ flow, const uint8_t* __restrict__ valid,
                                                        uint8_t* __restrict__ warped, int h, int w,
                                                        unsigned long long* __restrict__ partial) {
    __shared__ unsigned int red[4 * 256];
    const size_t hw = (size_t)h * w;
    const int tid = threadIdx.x;
    unsigned int s[4] = {0u, 0u, 0u, 0u};
    for (int j = 0; j < L1_PER_THREAD; ++j) {
        const size_t at = (size_t)blockIdx.x * L1_BLOCK_PIXELS + (size_t)j * 256 + tid;
        if (at >= hw) break;
        size_t from = at;
        if (flow) {
            const int y = (int)(at / w), x = (int)(at % w);
            from = (size_t)warp_index(y, flow[hw + at], h) * w + warp_index(x, flow[at], w);
        }
        const uint8_t* p = a + from * 3;
        const uint8_t* q = b + at * 3;
        if (valid[at]) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int d = (int)p[c] - (int)q[c];
                s[c] += (unsigned int)(d < 0 ? -d : d);
            }
            s[3] += 1u;
        }
        if (warped) {
            uint8_t* o = warped + at * 3;
            o[0] = p[0], o[1] = p[1], o[2] = p[2];
        }
    }
    block_tree4(red, s, tid);
    if (tid < 3)
        partial[(size_t)blockIdx.x * 3 + tid] =
            (unsigned long long)red[tid * 256] | (tid == 0 ? (unsigned long long)red[3 * 256] << 32 : 0ull);
}

__global__ __launch_bounds__(256) void l1_masked_sum_kernel(const unsigned long long* __restrict__ partial, size_t blocks,
                                                            double pixels, double* __restrict__ loss4) {
    __shared__ unsigned long long red[4 * 256];
    const int tid = threadIdx.x;
    unsigned long long s[4] = {0ull, 0ull, 0ull, 0ull};
    for (size_t t = tid; t < blocks; t += 256) {
        const unsigned long long first = partial[t * 3];
        s[0] += first & 0xffffffffull, s[3] += first >> 32;
        s[1] += partial[t * 3 + 1], s[2] += partial[t * 3 + 2];
    }
    block_tree4(red, s, tid);
    if (tid < 4) {
        const unsigned long long count = red[3 * 256];
        double v = 0.0;
        if (count) v = tid < 3 ? (double)red[tid * 256] / (255.0 * (double)count) : (double)count / pixels;
        loss4[tid] = v;
    }
}

// ------------------------------------------------------------------------------------------------ host
int frame_check(int h, int w) {
    if (h < 8 || w < 8 || (int64_t)h * w > VST_MAX_FRAME_PIXELS) return VST_E_SHAPE;
    return VST_OK;
}

bool off_grid(const void* p, uintptr_t bytes) { return (((uintptr_t)p) & (bytes - 1)) != 0; }

bool overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return a && b && pa < pb + nb && pb < pa + na;
}

dim3 tiles(int h, int w) { return dim3((unsigned)((w + TW - 1) / TW), (unsigned)((h + TH - 1) / TH)); }

unsigned blocks256(size_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace

int vst_flow_workspace_bytes(int h, int w, int levels, size_t* bytes) {
    if (!bytes) return VST_E_ARG;
    const int rc = frame_check(h, w);
    if (rc != VST_OK) return rc;
    if (levels < 1 || levels > MAX_LEVELS) return VST_E_SHAPE;
    *bytes = workspace_doubles(make_pyramid(h, w, levels)) * sizeof(double);
    return VST_OK;
}

int vst_flow_lk_u8(const uint8_t* ref_u8_hwc, const uint8_t* src_u8_hwc, int h, int w, int levels, int iters, int radius,
                   double lambda, float* flow_f32, void* ws, void* stream) {
    if (!ref_u8_hwc || !src_u8_hwc || !flow_f32 || !ws) return VST_E_ARG;
    const int rc = frame_check(h, w);
    if (rc != VST_OK) return rc;
    if (levels < 1 || levels > MAX_LEVELS || iters < 1 || iters > VST_FLOW_MAX_ITERS || radius < 1 || radius > RMAX) return VST_E_SHAPE;
    if (!(lambda > 0.0) || !(lambda < INFINITY)) return VST_E_ARG;
    const Pyramid p = make_pyramid(h, w, levels);
    const size_t n0 = (size_t)h * w, ws_bytes = workspace_doubles(p) * sizeof(double);
    if (off_grid(ws, 8) || off_grid(flow_f32, 4)) return VST_E_ARG;
    if (overlap(flow_f32, n0 * 8, ws, ws_bytes) || overlap(flow_f32, n0 * 8, ref_u8_hwc, n0 * 3) ||
        overlap(flow_f32, n0 * 8, src_u8_hwc, n0 * 3) || overlap(ws, ws_bytes, ref_u8_hwc, n0 * 3) ||
        overlap(ws, ws_bytes, src_u8_hwc, n0 * 3))
        return VST_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    double* base = (double*)ws;
    double* R = base;
    double* S = R + p.pixels;
    double* DX = S + p.pixels;
    double* DY = DX + p.pixels;
    double* tx = DY + p.pixels;
    double* ty = tx + n0;
    double* Rx = ty + n0;
    double* Ry = Rx + n0;
    double* A11 = Ry + n0;
    double* A12 = A11 + n0;
    double* A22 = A12 + n0;

    grey_kernel<<<dim3(blocks256(n0), 2), 256, 0, st>>>(ref_u8_hwc, src_u8_hwc, R, S, n0);
    VST_RETURN_IF_LAUNCH_FAILED();
    for (int l = 1; l < p.n; ++l) {
        down_kernel<<<dim3(blocks256((size_t)p.h[l] * p.w[l]), 2), 256, 0, st>>>(R + p.at[l - 1], S + p.at[l - 1], R + p.at[l],
                                                                                 S + p.at[l], p.h[l - 1], p.w[l - 1], p.h[l], p.w[l]);
        VST_RETURN_IF_LAUNCH_FAILED();
    }
    for (int l = p.n - 1; l >= 0; --l) {
        const int lh = p.h[l], lw = p.w[l];
        const size_t ln = (size_t)lh * lw;
        double* dx = DX + p.at[l];
        double* dy = DY + p.at[l];
        if (l == p.n - 1) {
            hipError_t e = hipMemsetAsync(dx, 0, ln * sizeof(double), st);
            if (e == hipSuccess) e = hipMemsetAsync(dy, 0, ln * sizeof(double), st);
            if (e != hipSuccess) return (int)e;
        } else {
            up_kernel<<<dim3(blocks256(ln), 2), 256, 0, st>>>(DX + p.at[l + 1], DY + p.at[l + 1], dx, dy, lh, lw, p.h[l + 1],
                                                              p.w[l + 1]);
            VST_RETURN_IF_LAUNCH_FAILED();
        }
        tensor_kernel<<<tiles(lh, lw), THREADS, 0, st>>>(R + p.at[l], Rx, Ry, A11, A12, A22, lh, lw, radius, lambda);
        VST_RETURN_IF_LAUNCH_FAILED();
        for (int it = 0; it < iters; ++it) {
            lk_iter_kernel<<<tiles(lh, lw), THREADS, 0, st>>>(R + p.at[l], S + p.at[l], Rx, Ry, A11, A12, A22, dx, dy, tx, ty, lh,
                                                              lw, radius);
            VST_RETURN_IF_LAUNCH_FAILED();
            smooth_kernel<<<tiles(lh, lw), THREADS, 0, st>>>(tx, ty, dx, dy, (l == 0 && it == iters - 1) ? flow_f32 : nullptr, lh,
                                                             lw);
            VST_RETURN_IF_LAUNCH_FAILED();
        }
    }
    return VST_OK;
}

int vst_flow_consistency(const float* flow_fwd, const float* flow_bwd, int h, int w, uint8_t* valid, void* stream) {
    if (!flow_fwd || !flow_bwd || !valid) return VST_E_ARG;
    const int rc = frame_check(h, w);
    if (rc != VST_OK) return rc;
    const size_t n = (size_t)h * w;
    if (off_grid(flow_fwd, 4) || off_grid(flow_bwd, 4) || overlap(valid, n, flow_fwd, n * 8) || overlap(valid, n, flow_bwd, n * 8))
        return VST_E_ARG;
    consistency_kernel<<<blocks256(n), 256, 0, (hipStream_t)stream>>>(flow_fwd, flow_bwd, valid, h, w);
    VST_RETURN_IF_LAUNCH_FAILED();
    return VST_OK;
}

int vst_temporal_l1_masked_u8(const uint8_t* a_u8_hwc, const uint8_t* b_u8_hwc, const float* flow_or_null, const uint8_t* valid,
                              int h, int w, double* loss4, uint8_t* warped_or_null, void* ws, void* stream) {
    if (!a_u8_hwc || !b_u8_hwc || !valid || !loss4 || !ws || warped_or_null == a_u8_hwc || warped_or_null == b_u8_hwc ||
        warped_or_null == valid)
        return VST_E_ARG;
    const int rc = frame_check(h, w);
    if (rc != VST_OK) return rc;
    if (off_grid(ws, 8) || off_grid(loss4, 8) || off_grid(flow_or_null, 4)) return VST_E_ARG;
    const size_t n = (size_t)h * w, blocks = (n + L1_BLOCK_PIXELS - 1) / L1_BLOCK_PIXELS;
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* partial = (unsigned long long*)ws;
    l1_masked_kernel<<<(unsigned)blocks, 256, 0, st>>>(a_u8_hwc, b_u8_hwc, flow_or_null, valid, warped_or_null, h, w, partial);
    VST_RETURN_IF_LAUNCH_FAILED();
    l1_masked_sum_kernel<<<1, 256, 0, st>>>(partial, blocks, (double)n, loss4);
    VST_RETURN_IF_LAUNCH_FAILED();
    return VST_OK;
}
