// Guided upscale (vstnet.h, "Guided upscale"): He and Sun's fast guided filter with a colour guide.  The fit
// runs at the working size - window moments of the guide and of the stylised frame, a 3x3 solve per pixel, a box mean of the 12
// coefficient planes - in fp64; the apply samples the planes bilinearly at the full size and applies them to the source frame.
// The box sums are separable, one pass per axis, each a plain sum over the clipped window (no running sum: nothing is subtracted
// anywhere), through a workspace of doubles the caller owns.
#include "common.h"
#include <math.h>

namespace {

constexpr int MOMENTS = 21;         // I (3), p (3), I I^T (6: 00 01 02 11 12 22), I p^T (9: 3 k + c)
constexpr int COEFS = 12;           // A[k][c] at plane 3 k + c, b[c] at plane 9 + c

// ------------------------------------------------------------------------------------------------ fit
// Stage 1: the vertical window sums of the 21 moment planes.  One thread per working-size pixel; a workgroup is 256 columns of
// one row.  The products are formed in double from I = guide / 255 and the fp32 target.  The vertical pass comes first because it
// is the one whose window rows are different cache lines: here they are rows of the 15-byte-per-pixel inputs, not of the 168-byte-
// per-pixel sums (the horizontal pass behind it reads neighbours inside the lines its own wave has just touched).
__global__ __launch_bounds__(256) void guided_moments_v_kernel(const uint8_t* __restrict__ guide, const float* __restrict__ target,
                                                               double* __restrict__ out, int h, int w, int r, int col_blocks) {
    const int y = blockIdx.x / col_blocks;
    const int x = (blockIdx.x % col_blocks) * 256 + threadIdx.x;
    if (x >= w) return;
    const int ya = y - r < 0 ? 0 : y - r, yb = y + r > h - 1 ? h - 1 : y + r;
    const size_t hw = (size_t)h * w, row = (size_t)y * w;
    double s[MOMENTS];
#pragma unroll
    for (int n = 0; n < MOMENTS; ++n) s[n] = 0.0;
    for (int j = ya; j <= yb; ++j) {
        const size_t at = (size_t)j * w + x;
        const uint8_t* g = guide + at * 3;
        const double i0 = (double)g[0] / 255.0, i1 = (double)g[1] / 255.0, i2 = (double)g[2] / 255.0;
        const double p0 = (double)target[at], p1 = (double)target[hw + at], p2 = (double)target[2 * hw + at];
        s[0] += i0, s[1] += i1, s[2] += i2;
        s[3] += p0, s[4] += p1, s[5] += p2;
        s[6] += i0 * i0, s[7] += i0 * i1, s[8] += i0 * i2, s[9] += i1 * i1, s[10] += i1 * i2, s[11] += i2 * i2;
        s[12] += i0 * p0, s[13] += i0 * p1, s[14] += i0 * p2;
        s[15] += i1 * p0, s[16] += i1 * p1, s[17] += i1 * p2;
        s[18] += i2 * p0, s[19] += i2 * p1, s[20] += i2 * p2;
    }
#pragma unroll
    for (int n = 0; n < MOMENTS; ++n) out[n * hw + row + x] = s[n];
}

// Stage 2: the horizontal sums of stage 1's planes, the means over the clipped box, and the solve A = (Sigma + eps 1)^-1 C by the
// cofactors of the symmetric 3x3 (its condition is at most (lambda_max + eps) / eps, far inside fp64), b = mean_p - A^T mean_I.
__global__ __launch_bounds__(256) void guided_solve_h_kernel(const double* __restrict__ sums, double* __restrict__ ab, int h, int w,
                                                             int r, double eps, int col_blocks) {
    const int y = blockIdx.x / col_blocks;
    const int x = (blockIdx.x % col_blocks) * 256 + threadIdx.x;
    if (x >= w) return;
    const int xa = x - r < 0 ? 0 : x - r, xb = x + r > w - 1 ? w - 1 : x + r;
    const int ya = y - r < 0 ? 0 : y - r, yb = y + r > h - 1 ? h - 1 : y + r;
    const size_t hw = (size_t)h * w;
    double s[MOMENTS];
#pragma unroll
    for (int n = 0; n < MOMENTS; ++n) s[n] = 0.0;
    for (int j = xa; j <= xb; ++j) {
        const double* p = sums + (size_t)y * w + j;
#pragma unroll
        for (int n = 0; n < MOMENTS; ++n) s[n] += p[n * hw];
    }
    const double inv_n = 1.0 / (double)((xb - xa + 1) * (yb - ya + 1));
#pragma unroll
    for (int n = 0; n < MOMENTS; ++n) s[n] *= inv_n;
    const double mi0 = s[0], mi1 = s[1], mi2 = s[2];
    const double m00 = s[6] - mi0 * mi0 + eps, m01 = s[7] - mi0 * mi1, m02 = s[8] - mi0 * mi2;
    const double m11 = s[9] - mi1 * mi1 + eps, m12 = s[10] - mi1 * mi2, m22 = s[11] - mi2 * mi2 + eps;
    const double c00 = m11 * m22 - m12 * m12, c01 = m02 * m12 - m01 * m22, c02 = m01 * m12 - m02 * m11;
    const double c11 = m00 * m22 - m02 * m02, c12 = m01 * m02 - m00 * m12, c22 = m00 * m11 - m01 * m01;
    const double inv_det = 1.0 / (m00 * c00 + m01 * c01 + m02 * c02);
    double* o = ab + (size_t)y * w + x;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double mp = s[3 + c];
        const double v0 = s[12 + c] - mi0 * mp, v1 = s[15 + c] - mi1 * mp, v2 = s[18 + c] - mi2 * mp;    // cov(I_k, p_c)
        const double a0 = (c00 * v0 + c01 * v1 + c02 * v2) * inv_det;
        const double a1 = (c01 * v0 + c11 * v1 + c12 * v2) * inv_det;
        const double a2 = (c02 * v0 + c12 * v1 + c22 * v2) * inv_det;
        o[(0 + c) * hw] = a0, o[(3 + c) * hw] = a1, o[(6 + c) * hw] = a2;
        o[(9 + c) * hw] = mp - (a0 * mi0 + a1 * mi1 + a2 * mi2);
    }
}

// Stages 3 and 4: the box mean of the 12 planes of A and b.  One thread per plane value; a workgroup is 256 columns of one row of
// one plane (blockIdx.x = (plane * h + y) * col_blocks + column block).
__global__ __launch_bounds__(256) void guided_box_h_kernel(const double* __restrict__ src, double* __restrict__ dst, int w, int r,
                                                           int col_blocks) {
    const size_t row = blockIdx.x / col_blocks;                 // plane * h + y
    const int x = (blockIdx.x % col_blocks) * 256 + threadIdx.x;
    if (x >= w) return;
    const int xa = x - r < 0 ? 0 : x - r, xb = x + r > w - 1 ? w - 1 : x + r;
    const double* s = src + row * w;
    double acc = 0.0;
    for (int j = xa; j <= xb; ++j) acc += s[j];
    dst[row * w + x] = acc;
}

__global__ __launch_bounds__(256) void guided_box_v_kernel(const double* __restrict__ src, float* __restrict__ coef, int h, int w,
                                                           int r, int col_blocks) {
    const size_t row = blockIdx.x / col_blocks;                 // plane * h + y
    const int x = (blockIdx.x % col_blocks) * 256 + threadIdx.x;
    if (x >= w) return;
    const size_t plane = row / h;
    const int y = (int)(row - plane * h);
    const int xa = x - r < 0 ? 0 : x - r, xb = x + r > w - 1 ? w - 1 : x + r;
    const int ya = y - r < 0 ? 0 : y - r, yb = y + r > h - 1 ? h - 1 : y + r;
    const double* s = src + plane * h * w + x;
    double acc = 0.0;
    for (int j = ya; j <= yb; ++j) acc += s[(size_t)j * w];
    coef[row * w + x] = (float)(acc / (double)((xb - xa + 1) * (yb - ya + 1)));
}

// ------------------------------------------------------------------------------------------------ apply
// Where a full-size coordinate falls on the working grid: half-pixel centres, clamped to the grid, in double (a frame is wider
// than fp32 resolves to a useful fraction), the fraction rounded to fp32 once.
struct Tap {
    int i0, i1;         // the two working-size indices
    float f;            // the weight of i1
};
__device__ __forceinline__ Tap tap_of(int X, int n_small, double ratio /* n_small / n_full */) {
    double v = ((double)X + 0.5) * ratio - 0.5;
    v = v < 0.0 ? 0.0 : v;
    const double top = (double)(n_small - 1);
    v = v > top ? top : v;
    Tap t;
    t.i0 = (int)v;
    t.i1 = t.i0 + 1 < n_small ? t.i0 + 1 : n_small - 1;
    t.f = (float)(v - (double)t.i0);
    return t;
}

// one coefficient plane at (ty, tx): the four neighbours under fp32 weights
__device__ __forceinline__ float bilinear(const float* __restrict__ plane, int w, const Tap& ty, const Tap& tx) {
    const float* r0 = plane + (size_t)ty.i0 * w;
    const float* r1 = plane + (size_t)ty.i1 * w;
    const float top = fmaf(tx.f, r0[tx.i1] - r0[tx.i0], r0[tx.i0]);
    const float bot = fmaf(tx.f, r1[tx.i1] - r1[tx.i0], r1[tx.i0]);
    return fmaf(ty.f, bot - top, top);
}

// q_c = b_c + sum_k A[k][c] I_k of one pixel and channel
__device__ __forceinline__ float guided_value(const float* __restrict__ coef, size_t hw, int w, int c, const Tap& ty, const Tap& tx,
                                              float i0, float i1, float i2) {
    const float* p = coef + c * hw;
    float q = bilinear(p + 9 * hw, w, ty, tx);
    q = fmaf(bilinear(p, w, ty, tx), i0, q);
    q = fmaf(bilinear(p + 3 * hw, w, ty, tx), i1, q);
    q = fmaf(bilinear(p + 6 * hw, w, ty, tx), i2, q);
    return q;
}

// The u8 form.  A workgroup is 256 pixels (768 bytes) of one output row.  Thread t computes the three values of pixel x0 + t, so
// that a wave's coefficient reads are consecutive addresses of one plane (were a thread to compute its own 4 bytes, neighbouring
// lanes would sit in different channels and every load would touch three planes' lines), and leaves its 3 bytes in LDS.  Then a
// thread owns 4 consecutive output bytes, on the destination's dword grid, and stores them as one dword; only a block's ragged
// first and last dword - a row is 3 W bytes: no multiple of 4 in general - go out byte by byte.  The row's vertical tap is uniform.
__global__ __launch_bounds__(256) void guided_apply_u8_kernel(const float* __restrict__ coef, int h, int w,
                                                              const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int H, int W,
                                                              int col_blocks) {
    __shared__ uint8_t bytes[768];
    const int Y = blockIdx.x / col_blocks;
    const int x0 = (blockIdx.x % col_blocks) * 256;
    const int npix = W - x0 < 256 ? W - x0 : 256;
    const int t = threadIdx.x;
    if (t < npix) {
        const size_t hw = (size_t)h * w;
        const Tap ty = tap_of(Y, h, (double)h / H), tx = tap_of(x0 + t, w, (double)w / W);
        const uint8_t* s = src + ((size_t)Y * W + x0 + t) * 3;
        const float i0 = (float)s[0] / 255.f, i1 = (float)s[1] / 255.f, i2 = (float)s[2] / 255.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float v = guided_value(coef, hw, w, c, ty, tx, i0, i1, i2) * 255.f;
            // clamp(0, 255) then truncation; NaN -> 0 by the first test, not by what a conversion makes of a NaN
            bytes[3 * t + c] = (uint8_t)(unsigned)(v > 0.f ? (v > 255.f ? 255.f : v) : 0.f);
        }
    }
    __syncthreads();
    uint8_t* base = dst + ((size_t)Y * W + x0) * 3;          // the block's first byte, `a` bytes into a dword of the destination
    const int nbytes = 3 * npix;
    const int a = (int)(((uintptr_t)base) & 3);
    const int lo = 4 * t - a;                                // dword t of the block covers its bytes [lo, lo + 4): at most 193 dwords
    if (lo >= nbytes) return;
    if (lo >= 0 && lo + 4 <= nbytes) {
        *(unsigned*)(base + lo) = (unsigned)bytes[lo] | (unsigned)bytes[lo + 1] << 8 | (unsigned)bytes[lo + 2] << 16 |
                                  (unsigned)bytes[lo + 3] << 24;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (lo + i >= 0 && lo + i < nbytes) base[lo + i] = bytes[lo + i];
    }
}

// The f32 form: one thread per full-size pixel, three planar stores.
__global__ __launch_bounds__(256) void guided_apply_f32_kernel(const float* __restrict__ coef, int h, int w,
                                                               const uint8_t* __restrict__ src, float* __restrict__ dst, int H, int W,
                                                               int col_blocks) {
    const int Y = blockIdx.x / col_blocks;
    const int X = (blockIdx.x % col_blocks) * 256 + threadIdx.x;
    if (X >= W) return;
    const size_t hw = (size_t)h * w, HW = (size_t)H * W;
    const Tap ty = tap_of(Y, h, (double)h / H), tx = tap_of(X, w, (double)w / W);
    const uint8_t* s = src + ((size_t)Y * W + X) * 3;
    const float i0 = (float)s[0] / 255.f, i1 = (float)s[1] / 255.f, i2 = (float)s[2] / 255.f;
    float* d = dst + (size_t)Y * W + X;
#pragma unroll
    for (int c = 0; c < 3; ++c) d[c * HW] = guided_value(coef, hw, w, c, ty, tx, i0, i1, i2);
}

// ------------------------------------------------------------------------------------------------ host: checks
// the coefficient planes are addressed in bytes below 2^31 (12 planes of floats), and so is everything smaller at that size
int fit_check(int h, int w, int radius) {
    if (h <= 0 || w <= 0) return VST_E_ARG;
    if (radius < 1 || radius > VST_GUIDED_MAX_RADIUS) return VST_E_SHAPE;
    if ((int64_t)h * w * COEFS * (int64_t)sizeof(float) > 0x7fffffffLL) return VST_E_SHAPE;
    return VST_OK;
}

int apply_check(const float* coef, int h, int w, const uint8_t* src, int H, int W, const void* dst, int dst_elem_bytes) {
    if (!coef || !src || !dst || h <= 0 || w <= 0 || H <= 0 || W <= 0) return VST_E_ARG;
    if ((((uintptr_t)coef) & 3) != 0 || (((uintptr_t)dst) & (uintptr_t)(dst_elem_bytes - 1)) != 0) return VST_E_ARG;
    if (H < h || W < w) return VST_E_SHAPE;
    if ((int64_t)h * w * COEFS * (int64_t)sizeof(float) > 0x7fffffffLL) return VST_E_SHAPE;
    if ((int64_t)H * W * 3 * dst_elem_bytes > 0x7fffffffLL) return VST_E_SHAPE;
    return VST_OK;
}

}  // namespace

int vst_guided_workspace_bytes(int h, int w, int radius, size_t* bytes) {
    if (!bytes) return VST_E_ARG;
    const int rc = fit_check(h, w, radius);
    if (rc != VST_OK) return rc;
    *bytes = (size_t)h * w * (MOMENTS + COEFS) * sizeof(double);
    return VST_OK;
}

int vst_guided_fit(const uint8_t* guide_u8_hwc, const float* target_f32_planar, int h, int w, int radius, double eps, float* coef_f32,
                   void* ws, void* stream) {
    if (!guide_u8_hwc || !target_f32_planar || !coef_f32) return VST_E_ARG;
    const int rc = fit_check(h, w, radius);
    if (rc != VST_OK) return rc;
    if (!(eps > 0.0) || !(eps < INFINITY)) return VST_E_ARG;
    if (!ws) return VST_E_WORKSPACE;
    if ((((uintptr_t)ws) & 7) != 0 || ((((uintptr_t)target_f32_planar) | ((uintptr_t)coef_f32)) & 3) != 0) return VST_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    const size_t hw = (size_t)h * w;
    double* sums = (double*)ws;                 // [21][h][w]: stage 1's sums, then stage 3's (12 planes)
    double* ab = sums + MOMENTS * hw;           // [12][h][w]: A and b before the smoothing
    const int col_blocks = (w + 255) / 256;
    const int64_t blocks = (int64_t)col_blocks * h;
    if (blocks * COEFS > 0x7fffffffLL) return VST_E_SHAPE;
    guided_moments_v_kernel<<<(unsigned)blocks, 256, 0, st>>>(guide_u8_hwc, target_f32_planar, sums, h, w, radius, col_blocks);
    VST_RETURN_IF_LAUNCH_FAILED();
    guided_solve_h_kernel<<<(unsigned)blocks, 256, 0, st>>>(sums, ab, h, w, radius, eps, col_blocks);
    VST_RETURN_IF_LAUNCH_FAILED();
    guided_box_h_kernel<<<(unsigned)(blocks * COEFS), 256, 0, st>>>(ab, sums, w, radius, col_blocks);
    VST_RETURN_IF_LAUNCH_FAILED();
    guided_box_v_kernel<<<(unsigned)(blocks * COEFS), 256, 0, st>>>(sums, coef_f32, h, w, radius, col_blocks);
    VST_RETURN_IF_LAUNCH_FAILED();
    return VST_OK;
}

int vst_guided_apply_u8(const float* coef, int h, int w, const uint8_t* src_u8_hwc, int H, int W, uint8_t* dst_u8_hwc, void* stream) {
    const int rc = apply_check(coef, h, w, src_u8_hwc, H, W, dst_u8_hwc, 1);
    if (rc != VST_OK) return rc;
    const int col_blocks = (W + 255) / 256;
    if ((int64_t)col_blocks * H > 0x7fffffffLL) return VST_E_SHAPE;
    guided_apply_u8_kernel<<<(unsigned)(col_blocks * H), 256, 0, (hipStream_t)stream>>>(coef, h, w, src_u8_hwc, dst_u8_hwc, H, W,
                                                                                         col_blocks);
    VST_RETURN_IF_LAUNCH_FAILED();
    return VST_OK;
}

int vst_guided_apply_f32(const float* coef, int h, int w, const uint8_t* src_u8_hwc, int H, int W, float* dst_f32_planar, void* stream) {
    const int rc = apply_check(coef, h, w, src_u8_hwc, H, W, dst_f32_planar, 4);
    if (rc != VST_OK) return rc;
    const int col_blocks = (W + 255) / 256;
    if ((int64_t)col_blocks * H > 0x7fffffffLL) return VST_E_SHAPE;
    guided_apply_f32_kernel<<<(unsigned)(col_blocks * H), 256, 0, (hipStream_t)stream>>>(coef, h, w, src_u8_hwc, dst_f32_planar, H, W,
                                                                                          col_blocks);
    VST_RETURN_IF_LAUNCH_FAILED();
    return VST_OK;
}
