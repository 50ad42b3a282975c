// Matting-Laplacian affinity loss (vstnet.h, "Affinity loss"): x^T L x / (h w) per channel and, optionally,
// the gradient 2 L x / (h w), with L Levin's Matting Laplacian of the guide - without the matrix.  (L x)_i is the sum, over the
// (2r+1)^2 windows that hold pixel i and lie inside the image, of the residual at i of the window's ridge-regularised affine fit
// of x on the guide.  One workgroup takes a tile of pixels: it loads the tile and a 2r halo of guide and x into LDS as doubles,
// fits every window whose centre lies within r of the tile, keeps the fits in LDS, and then each pixel sums its residuals.
// Everything is fp64.  Moments are centred on the window's centre pixel, so a flat window's covariance and a constant x's
// residuals are exactly 0.  Partial sums leave by a fixed tree per workgroup and a second launch: no floating-point atomics.
#include "common.h"
#include <math.h>

namespace {

// The tile per radius.  LDS holds 6 doubles per pixel of the tile plus a 2r halo and 15 per fit of the tile plus an r halo:
//   r = 1: 16 x 16   20 * 20 * 48 + 18 * 18 * 120 = 58080 bytes
//   r = 2: 12 x 16   20 * 24 * 48 + 16 * 20 * 120 = 61440 bytes
//   r = 3: 10 x 12   22 * 24 * 48 + 16 * 18 * 120 = 59904 bytes
// each below 64 KB, so two workgroups are resident on a CU's 160 KB whatever the radius ("Affinity loss").
template <int R> struct MatTile {
    static constexpr int TH = R == 1 ? 16 : (R == 2 ? 12 : 10);
    static constexpr int TW = R == 3 ? 12 : 16;
    static constexpr int PH = TH + 4 * R, PW = TW + 4 * R;      // pixels held: origin (ty0 - 2r, tx0 - 2r)
    static constexpr int FH = TH + 2 * R, FW = TW + 2 * R;      // fits held: centres from (ty0 - r, tx0 - r)
    static constexpr int NPIX = PH * PW, NFIT = FH * FW;
    static constexpr int LDS_BYTES = (6 * NPIX + 15 * NFIT) * 8;
};
constexpr int FIT_PLANES = 15;      // mu (3), then per channel c: the window mean of x_c and a_c = inv v_c (3)

__host__ __device__ constexpr int mat_tile_h(int r) { return r == 1 ? 16 : (r == 2 ? 12 : 10); }
__host__ __device__ constexpr int mat_tile_w(int r) { return r == 3 ? 12 : 16; }

__device__ __forceinline__ void load_x(const float* __restrict__ x, size_t at, size_t hw, double* v) {
    v[0] = (double)x[at], v[1] = (double)x[hw + at], v[2] = (double)x[2 * hw + at];
}
__device__ __forceinline__ void load_x(const uint8_t* __restrict__ x, size_t at, size_t, double* v) {
    const uint8_t* p = x + at * 3;
    v[0] = (double)p[0] / 255.0, v[1] = (double)p[1] / 255.0, v[2] = (double)p[2] / 255.0;
}

template <int R, typename X>
__global__ __launch_bounds__(256) void matting_tile_kernel(const uint8_t* __restrict__ guide, const X* __restrict__ x, int h, int w,
                                                           double ridge /* eps / n */, double inv_hw, double* __restrict__ partial,
                                                           float* __restrict__ grad, int tiles_x) {
    using T = MatTile<R>;
    constexpr int D = 2 * R + 1, N = D * D;
    static_assert(T::TH * T::TW <= 256 && T::LDS_BYTES <= 65536 && 6 * T::NPIX >= 3 * 256, "tile");
    __shared__ double pix[6 * T::NPIX];             // [6][PH][PW]: I (3), x (3); after the residuals, the reduction's scratch
    __shared__ double fit[FIT_PLANES * T::NFIT];    // [15][FH][FW]
    const int tid = threadIdx.x;
    const int ty0 = (int)(blockIdx.x / tiles_x) * T::TH, tx0 = (int)(blockIdx.x % tiles_x) * T::TW;
    const size_t hw = (size_t)h * w;

    // ---- the tile and its halo.  Pixels outside the image are zeros nobody reads: only windows inside the image are fitted.
    for (int idx = tid; idx < T::NPIX; idx += 256) {
        const int gy = ty0 - 2 * R + idx / T::PW, gx = tx0 - 2 * R + idx % T::PW;
        double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (gy >= 0 && gy < h && gx >= 0 && gx < w) {
            const size_t at = (size_t)gy * w + gx;
            const uint8_t* g = guide + at * 3;
            v[0] = (double)g[0] / 255.0, v[1] = (double)g[1] / 255.0, v[2] = (double)g[2] / 255.0;
            load_x(x, at, hw, v + 3);
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) pix[k * T::NPIX + idx] = v[k];
    }
    __syncthreads();

    // ---- the fits: one window per thread and turn
    for (int idx = tid; idx < T::NFIT; idx += 256) {
        const int fy = idx / T::FW, fx = idx % T::FW;
        const int cy = ty0 - R + fy, cx = tx0 - R + fx;
        if (cy < R || cy > h - 1 - R || cx < R || cx > w - 1 - R) continue;
        const int first = fy * T::PW + fx;                      // the window's first pixel in pix; its centre is R rows and columns on
        const int centre = first + R * T::PW + R;
        double c[6], m[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) c[k] = pix[k * T::NPIX + centre], m[k] = 0.0;
        for (int j = 0; j < D; ++j)
            for (int i = 0; i < D; ++i) {
                const int at = first + j * T::PW + i;
#pragma unroll
                for (int k = 0; k < 6; ++k) m[k] += pix[k * T::NPIX + at] - c[k];
            }
#pragma unroll
        for (int k = 0; k < 6; ++k) m[k] *= 1.0 / (double)N;    // the means, relative to the centre pixel
        double s00 = 0.0, s01 = 0.0, s02 = 0.0, s11 = 0.0, s12 = 0.0, s22 = 0.0, v[3][3] = {};
        for (int j = 0; j < D; ++j)
            for (int i = 0; i < D; ++i) {
                const int at = first + j * T::PW + i;
                double d[6];
#pragma unroll
                for (int k = 0; k < 6; ++k) d[k] = (pix[k * T::NPIX + at] - c[k]) - m[k];
                s00 += d[0] * d[0], s01 += d[0] * d[1], s02 += d[0] * d[2], s11 += d[1] * d[1], s12 += d[1] * d[2], s22 += d[2] * d[2];
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) v[ch][0] += d[0] * d[3 + ch], v[ch][1] += d[1] * d[3 + ch], v[ch][2] += d[2] * d[3 + ch];
            }
        const double inv_n = 1.0 / (double)N;
        const double m00 = s00 * inv_n + ridge, m01 = s01 * inv_n, m02 = s02 * inv_n;
        const double m11 = s11 * inv_n + ridge, m12 = s12 * inv_n, m22 = s22 * inv_n + ridge;
        // M = L D L^T and two triangular solves per channel.  M is positive definite (the ridge), so no pivoting; the error
        // grows with M's condition, (lambda_max + eps / n) / (eps / n), where the cofactor inverse of guided.hip, whose ridge is
        // 1e-3 and not 1e-8, would pay its square: a window across an edge between two flat regions has rank one.
        const double i0 = 1.0 / m00;
        const double l10 = m01 * i0, l20 = m02 * i0;
        const double t12 = m12 - l20 * m01;
        const double i1 = 1.0 / (m11 - l10 * m01);
        const double l21 = t12 * i1;
        const double i2 = 1.0 / (m22 - l20 * m02 - l21 * t12);
#pragma unroll
        for (int k = 0; k < 3; ++k) fit[k * T::NFIT + idx] = c[k] + m[k];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const double z0 = v[ch][0] * inv_n;                             // cov(I, x_c), then forward substitution
            const double z1 = v[ch][1] * inv_n - l10 * z0;
            const double z2 = v[ch][2] * inv_n - l20 * z0 - l21 * z1;
            const double a2 = z2 * i2;
            const double a1 = z1 * i1 - l21 * a2;
            const double a0 = z0 * i0 - l10 * a1 - l20 * a2;
            double* f = fit + (3 + 4 * ch) * T::NFIT + idx;
            f[0] = c[3 + ch] + m[3 + ch];
            f[T::NFIT] = a0, f[2 * T::NFIT] = a1, f[3 * T::NFIT] = a2;
        }
    }
    __syncthreads();

    // ---- the residuals: one pixel of the tile per thread
    double share[3] = {0.0, 0.0, 0.0};
    const int ly = tid / T::TW, lx = tid % T::TW;
    const int y = ty0 + ly, xx = tx0 + lx;
    if (tid < T::TH * T::TW && y < h && xx < w) {
        const int at = (ly + 2 * R) * T::PW + lx + 2 * R;
        double p[6], acc[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < 6; ++k) p[k] = pix[k * T::NPIX + at];
        for (int dy = -R; dy <= R; ++dy) {
            const int cy = y + dy;
            if (cy < R || cy > h - 1 - R) continue;
            for (int dx = -R; dx <= R; ++dx) {
                const int cx = xx + dx;
                if (cx < R || cx > w - 1 - R) continue;
                const double* f = fit + (ly + R + dy) * T::FW + lx + R + dx;
                const double d0 = p[0] - f[0], d1 = p[1] - f[T::NFIT], d2 = p[2] - f[2 * T::NFIT];
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    const double* a = f + (3 + 4 * ch) * T::NFIT;
                    acc[ch] += (p[3 + ch] - a[0]) - (d0 * a[T::NFIT] + d1 * a[2 * T::NFIT] + d2 * a[3 * T::NFIT]);
                }
            }
        }
        const size_t g = (size_t)y * w + xx;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            share[ch] = p[3 + ch] * acc[ch];
            if (grad) grad[ch * hw + g] = (float)(2.0 * acc[ch] * inv_hw);
        }
    }
    __syncthreads();                                // every read of pix is done: it becomes the tree's scratch
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) pix[ch * 256 + tid] = share[ch];
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) pix[ch * 256 + tid] += pix[ch * 256 + tid + s];
        }
        __syncthreads();
    }
    if (tid < 3) partial[(size_t)blockIdx.x * 3 + tid] = pix[tid * 256];
}

// The second stage: one workgroup adds the workgroups' partial sums, thread t those of tiles t, t + 256, ... in that order, then
// the same fixed tree; loss3[c] = sum / (h w).
__global__ __launch_bounds__(256) void matting_sum_kernel(const double* __restrict__ partial, size_t tiles, double hw,
                                                          double* __restrict__ loss3) {
    __shared__ double red[3 * 256];
    const int tid = threadIdx.x;
    double s[3] = {0.0, 0.0, 0.0};
    for (size_t t = tid; t < tiles; t += 256) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) s[ch] += partial[t * 3 + ch];
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) red[ch * 256 + tid] = s[ch];
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if (tid < k) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) red[ch * 256 + tid] += red[ch * 256 + tid + k];
        }
        __syncthreads();
    }
    if (tid < 3) loss3[tid] = red[tid * 256] / hw;
}

// ------------------------------------------------------------------------------------------------ host
int shape_check(int h, int w, int radius) {
    if (radius < 1 || radius > VST_MATTING_MAX_RADIUS) return VST_E_SHAPE;
    if (h < 2 * radius + 1 || w < 2 * radius + 1 || (int64_t)h * w > VST_MAX_FRAME_PIXELS) return VST_E_SHAPE;
    return VST_OK;
}

size_t tile_count(int h, int w, int radius, int* tiles_x) {
    const int th = mat_tile_h(radius), tw = mat_tile_w(radius);
    *tiles_x = (w + tw - 1) / tw;
    return (size_t)((h + th - 1) / th) * (size_t)*tiles_x;
}

template <typename X>
int matting_loss(const uint8_t* guide, const X* x, int h, int w, int radius, double eps, double* loss3, float* grad, void* ws,
                 hipStream_t st) {
    if (!guide || !x || !loss3 || !ws) return VST_E_ARG;
    const int rc = shape_check(h, w, radius);
    if (rc != VST_OK) return rc;
    if (!(eps > 0.0) || !(eps < INFINITY)) return VST_E_ARG;
    if (((((uintptr_t)ws) | ((uintptr_t)loss3)) & 7) != 0 || (((uintptr_t)grad) & 3) != 0 ||
        (((uintptr_t)x) & (uintptr_t)(sizeof(X) - 1)) != 0)
        return VST_E_ARG;
    int tiles_x = 0;
    const size_t tiles = tile_count(h, w, radius, &tiles_x);    // at most 2^26 / 120 + a ragged edge: far inside a grid's 2^31
    const int n = (2 * radius + 1) * (2 * radius + 1);
    const double hw = (double)h * (double)w;
    double* partial = (double*)ws;
    switch (radius) {
        case 1: matting_tile_kernel<1, X><<<(unsigned)tiles, 256, 0, st>>>(guide, x, h, w, eps / n, 1.0 / hw, partial, grad, tiles_x); break;
        case 2: matting_tile_kernel<2, X><<<(unsigned)tiles, 256, 0, st>>>(guide, x, h, w, eps / n, 1.0 / hw, partial, grad, tiles_x); break;
        default: matting_tile_kernel<3, X><<<(unsigned)tiles, 256, 0, st>>>(guide, x, h, w, eps / n, 1.0 / hw, partial, grad, tiles_x); break;
    }
    VST_RETURN_IF_LAUNCH_FAILED();
    matting_sum_kernel<<<1, 256, 0, st>>>(partial, tiles, hw, loss3);
    VST_RETURN_IF_LAUNCH_FAILED();
    return VST_OK;
}

}  // namespace

int vst_matting_workspace_bytes(int h, int w, int radius, size_t* bytes) {
    if (!bytes) return VST_E_ARG;
    const int rc = shape_check(h, w, radius);
    if (rc != VST_OK) return rc;
    int tiles_x = 0;
    *bytes = tile_count(h, w, radius, &tiles_x) * 3 * sizeof(double);
    return VST_OK;
}

int vst_matting_loss_f32(const uint8_t* guide_u8_hwc, const float* x_f32_planar, int h, int w, int radius, double eps, double* loss3,
                         float* grad_f32_planar_or_null, void* ws, void* stream) {
    return matting_loss(guide_u8_hwc, x_f32_planar, h, w, radius, eps, loss3, grad_f32_planar_or_null, ws, (hipStream_t)stream);
}

int vst_matting_loss_u8(const uint8_t* guide_u8_hwc, const uint8_t* x_u8_hwc, int h, int w, int radius, double eps, double* loss3,
                        float* grad_f32_planar_or_null, void* ws, void* stream) {
    return matting_loss(guide_u8_hwc, x_u8_hwc, h, w, radius, eps, loss3, grad_f32_planar_or_null, ws, (hipStream_t)stream);
}
