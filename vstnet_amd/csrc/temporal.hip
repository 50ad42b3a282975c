// Temporal loss (vstnet.h, "Temporal loss"): the reference's warp (grid_sample, nearest, border padding, with
// its W - 1 / align_corners=False quirk), mean |warp(a, flow) - b| per channel, and the smooth random flow it is measured under.
//
// The warp's index arithmetic is fp32 in the reference's order of operations with contraction OFF: the library is built at -O3,
// where a fused multiply-add would move the ties of the rounding to the nearest pixel.  The L1 sums are exact integers (uint8
// frames) or fp64 (float frames), leave each workgroup by a fixed tree and are added by a second launch in a fixed order: no
// floating-point atomics, the same bits on any stream.  The fake flow is fp64 throughout and rounded once to fp32.
#include "common.h"
#include <math.h>

namespace {

constexpr int L1_THREADS = 256;
constexpr int L1_PER_THREAD = 8;
constexpr int L1_BLOCK_PIXELS = L1_THREADS * L1_PER_THREAD;     // pixels one workgroup sums: one partial per channel each

// The source index along one axis of n pixels for destination p under flow flo: v = p - flo, normalised by max(n - 1, 1),
// un-normalised as align_corners=False does, clamped to the border, rounded to nearest with ties to even.  The last clamp is of
// the integer: a NaN flow must not index outside the frame.
__device__ __forceinline__ int warp_index(int p, float flo, int n) {
#pragma clang fp contract(off)
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

__device__ __forceinline__ size_t warp_source(const float* __restrict__ flow, int y, int x, int h, int w) {
    if (!flow) return (size_t)y * w + x;
    const size_t at = (size_t)y * w + x, hw = (size_t)h * w;
    const int sx = warp_index(x, flow[at], w), sy = warp_index(y, flow[hw + at], h);
    return (size_t)sy * w + sx;
}

__device__ __forceinline__ uint8_t noisy_u8(uint8_t v, float n) {
#pragma clang fp contract(off)
    float t = 255.0f * n;
    t = (float)v + t;
    t = rintf(t);
    return (uint8_t)fminf(fmaxf(t, 0.0f), 255.0f);
}

__global__ __launch_bounds__(256) void warp_u8_kernel(const uint8_t* __restrict__ src, const float* __restrict__ flow,
                                                      const float* __restrict__ noise, uint8_t* __restrict__ dst, int h, int w) {
    const size_t hw = (size_t)h * w;
    const size_t at = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (at >= hw) return;
    const int y = (int)(at / w), x = (int)(at % w);
    const uint8_t* s = src + warp_source(flow, y, x, h, w) * 3;
    uint8_t v[3] = {s[0], s[1], s[2]};
    if (noise) {
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = noisy_u8(v[c], noise[c * hw + at]);
    }
    uint8_t* d = dst + at * 3;
    d[0] = v[0], d[1] = v[1], d[2] = v[2];
}

__global__ __launch_bounds__(256) void warp_f32_kernel(const float* __restrict__ src, const float* __restrict__ flow,
                                                       const float* __restrict__ noise, float* __restrict__ dst, int h, int w) {
    const size_t hw = (size_t)h * w;
    const size_t at = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (at >= hw) return;
    const int y = (int)(at / w), x = (int)(at % w);
    const size_t from = warp_source(flow, y, x, h, w);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float v = src[c * hw + from];
        if (noise) v = v + noise[c * hw + at];
        dst[c * hw + at] = v;
    }
}

// ---- mean |warp(a) - b|.  Stage one: a workgroup sums L1_BLOCK_PIXELS pixels, thread t those at t, t + 256, ... of its span,
// then a fixed tree; three partials per workgroup.  Stage two: one workgroup adds the partials, thread t those of workgroups
// t, t + 256, ... in that order, then the same tree.
template <typename Acc>
__device__ __forceinline__ void block_tree3(Acc* red, Acc s0, Acc s1, Acc s2, int tid) {
    red[tid] = s0, red[256 + tid] = s1, red[512 + tid] = s2;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if (tid < k) {
#pragma unroll
            for (int c = 0; c < 3; ++c) red[c * 256 + tid] += red[c * 256 + tid + k];
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void l1_u8_kernel(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b,
                                                    const float* __restrict__ flow, uint8_t* __restrict__ warped, int h, int w,
                                                    unsigned long long* __restrict__ partial) {
    __shared__ unsigned int red[3 * 256];
    const size_t hw = (size_t)h * w;
    const int tid = threadIdx.x;
    unsigned int s[3] = {0u, 0u, 0u};                       // at most 8 x 255 per thread, 2048 x 255 per workgroup
    for (int j = 0; j < L1_PER_THREAD; ++j) {
        const size_t at = (size_t)blockIdx.x * L1_BLOCK_PIXELS + (size_t)j * 256 + tid;
        if (at >= hw) break;
        const int y = (int)(at / w), x = (int)(at % w);
        const uint8_t* p = a + warp_source(flow, y, x, h, w) * 3;
        const uint8_t* q = b + at * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int d = (int)p[c] - (int)q[c];
            s[c] += (unsigned int)(d < 0 ? -d : d);
        }
        if (warped) {
            uint8_t* o = warped + at * 3;
            o[0] = p[0], o[1] = p[1], o[2] = p[2];
        }
    }
    block_tree3(red, s[0], s[1], s[2], tid);
    if (tid < 3) partial[(size_t)blockIdx.x * 3 + tid] = red[tid * 256];
}

__global__ __launch_bounds__(256) void l1_f32_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                     const float* __restrict__ flow, float* __restrict__ warped, int h, int w,
                                                     double* __restrict__ partial) {
    __shared__ double red[3 * 256];
    const size_t hw = (size_t)h * w;
    const int tid = threadIdx.x;
    double s[3] = {0.0, 0.0, 0.0};
    for (int j = 0; j < L1_PER_THREAD; ++j) {
        const size_t at = (size_t)blockIdx.x * L1_BLOCK_PIXELS + (size_t)j * 256 + tid;
        if (at >= hw) break;
        const int y = (int)(at / w), x = (int)(at % w);
        const size_t from = warp_source(flow, y, x, h, w);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float v = a[c * hw + from];
            s[c] += fabs((double)v - (double)b[c * hw + at]);
            if (warped) warped[c * hw + at] = v;
        }
    }
    block_tree3(red, s[0], s[1], s[2], tid);
    if (tid < 3) partial[(size_t)blockIdx.x * 3 + tid] = red[tid * 256];
}

template <typename Acc>
__global__ __launch_bounds__(256) void l1_sum_kernel(const Acc* __restrict__ partial, size_t blocks, double denom,
                                                     double* __restrict__ loss3) {
    __shared__ Acc red[3 * 256];
    const int tid = threadIdx.x;
    Acc s[3] = {0, 0, 0};
    for (size_t t = tid; t < blocks; t += 256) {
#pragma unroll
        for (int c = 0; c < 3; ++c) s[c] += partial[t * 3 + c];
    }
    block_tree3(red, s[0], s[1], s[2], tid);
    if (tid < 3) loss3[tid] = (double)red[tid * 256] / denom;
}

// ---- the fake flow.  Both steps of the reference's construction are linear and separable: the bilinear upsample of the coarse
// grid G (cv2.resize, INTER_LINEAR) and the k x k box blur (cv2.blur, BORDER_REFLECT_101).  So
//     flow[c][y][x] = sum_gy By[y][gy] (sum_gx Bx[x][gx] G[gy][gx][c]) + shift[c]
// with Bx[x][gx] = (1 / k) sum over the k taps t of the upsample's weight of grid column gx at pixel reflect(x - k / 2 + t), and By
// alike.  The blur's k^2 taps per pixel become k taps per entry of two small tables, then gh multiply-adds per pixel.

__device__ __forceinline__ int reflect101(int i, int n) {     // one reflection is enough: k <= n, so |offset| <= n / 2
    if (i < 0) i = -i;
    if (i > n - 1) i = 2 * (n - 1) - i;
    return i < 0 ? 0 : (i > n - 1 ? n - 1 : i);
}

// The upsample's weight of coarse cell g at pixel d of an axis of dst pixels over src cells: source coordinate
// (d + 0.5) src / dst - 0.5, the two neighbours' weights, edges replicated.
__device__ __forceinline__ double linear_weight(int d, int g, int src, int dst) {
    const double s = ((double)d + 0.5) * (double)src / (double)dst - 0.5;
    int i0 = (int)floor(s);
    double f = s - (double)i0;
    if (i0 < 0) i0 = 0, f = 0.0;
    if (i0 >= src - 1) i0 = src - 1, f = 0.0;
    double wgt = 0.0;
    if (g == i0) wgt += 1.0 - f;
    if (g == i0 + 1) wgt += f;
    return wgt;
}

// tables: Bx [w][gw] then By [h][gh]; one thread per entry
__global__ __launch_bounds__(256) void flow_tables_kernel(double* __restrict__ tables, int h, int w, int gh, int gw, int ksize) {
    const size_t nx = (size_t)w * gw, ny = (size_t)h * gh;
    const size_t at = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (at >= nx + ny) return;
    const bool is_x = at < nx;
    const size_t e = is_x ? at : at - nx;
    const int n = is_x ? w : h, gn = is_x ? gw : gh;
    const int p = (int)(e / gn), g = (int)(e % gn);
    double s = 0.0;
    for (int t = 0; t < ksize; ++t) s += linear_weight(reflect101(p - ksize / 2 + t, n), g, gn, n);
    tables[at] = s / (double)ksize;
}

// rows: T [2][gh][w] = sum_gx Bx[x][gx] G[gy][gx][c]
__global__ __launch_bounds__(256) void flow_rows_kernel(const double* __restrict__ grid, const double* __restrict__ bx,
                                                        double* __restrict__ rows, int w, int gh, int gw) {
    const size_t n = (size_t)2 * gh * w;
    const size_t at = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (at >= n) return;
    const int x = (int)(at % w), gy = (int)((at / w) % gh), c = (int)(at / ((size_t)w * gh));
    double s = 0.0;
    for (int gx = 0; gx < gw; ++gx) s += bx[(size_t)x * gw + gx] * grid[((size_t)gy * gw + gx) * 2 + c];
    rows[at] = s;
}

__global__ __launch_bounds__(256) void flow_out_kernel(const double* __restrict__ rows, const double* __restrict__ by,
                                                       float* __restrict__ flow, int h, int w, int gh, double shift_x,
                                                       double shift_y) {
    const unsigned per_row = (unsigned)((w + 255) / 256);   // workgroups per row: a workgroup stays inside one row
    const int x = (int)((blockIdx.x % per_row) * 256 + threadIdx.x), y = (int)(blockIdx.x / per_row);
    if (x >= w) return;
    double s0 = 0.0, s1 = 0.0;
    for (int gy = 0; gy < gh; ++gy) {
        const double wy = by[(size_t)y * gh + gy];          // (the same address across the workgroup: a scalar load)
        s0 += wy * rows[(size_t)gy * w + x];
        s1 += wy * rows[((size_t)gh + gy) * w + x];
    }
    const size_t at = (size_t)y * w + x, hw = (size_t)h * w;
    flow[at] = (float)(s0 + shift_x);
    flow[hw + at] = (float)(s1 + shift_y);
}

// ------------------------------------------------------------------------------------------------ host
int frame_check(int h, int w) {
    if (h < 1 || w < 1 || (int64_t)h * w > VST_MAX_FRAME_PIXELS) return VST_E_SHAPE;
    return VST_OK;
}

bool off_grid(const void* p, uintptr_t bytes) { return (((uintptr_t)p) & (bytes - 1)) != 0; }

size_t l1_blocks(int h, int w) { return ((size_t)h * w + L1_BLOCK_PIXELS - 1) / L1_BLOCK_PIXELS; }

int flow_check(int h, int w, int gh, int gw, int ksize) {
    const int rc = frame_check(h, w);
    if (rc != VST_OK) return rc;
    if (gh < 1 || gw < 1 || gh > VST_FAKE_FLOW_MAX_GRID || gw > VST_FAKE_FLOW_MAX_GRID) return VST_E_SHAPE;
    if (ksize < 1 || ksize > (h < w ? h : w)) return VST_E_SHAPE;
    return VST_OK;
}

template <typename X, typename Acc>
int temporal_l1(const X* a, const X* b, const float* flow, int h, int w, double* loss3, X* warped, void* ws, double denom,
                hipStream_t st) {
    if (!a || !b || !loss3 || !ws || (const X*)warped == a || (const X*)warped == b) return VST_E_ARG;
    const int rc = frame_check(h, w);
    if (rc != VST_OK) return rc;
    if (off_grid(ws, 8) || off_grid(loss3, 8) || off_grid(flow, 4) || off_grid(a, sizeof(X)) || off_grid(b, sizeof(X)) ||
        off_grid(warped, sizeof(X)))
        return VST_E_ARG;
    const size_t blocks = l1_blocks(h, w);                  // at most 2^26 / 2048
    Acc* partial = (Acc*)ws;
    if constexpr (sizeof(X) == 1)
        l1_u8_kernel<<<(unsigned)blocks, 256, 0, st>>>(a, b, flow, warped, h, w, partial);
    else
        l1_f32_kernel<<<(unsigned)blocks, 256, 0, st>>>(a, b, flow, warped, h, w, partial);
    VST_RETURN_IF_LAUNCH_FAILED();
    l1_sum_kernel<Acc><<<1, 256, 0, st>>>(partial, blocks, denom, loss3);
    VST_RETURN_IF_LAUNCH_FAILED();
    return VST_OK;
}

template <typename X>
int warp_check(const X* src, const float* flow, const float* noise, X* dst, int h, int w) {
    if (!src || !dst || src == dst) return VST_E_ARG;
    const int rc = frame_check(h, w);
    if (rc != VST_OK) return rc;
    if (off_grid(flow, 4) || off_grid(noise, 4) || off_grid(src, sizeof(X)) || off_grid(dst, sizeof(X))) return VST_E_ARG;
    return VST_OK;
}

}  // namespace

int vst_warp_u8(const uint8_t* src_u8_hwc, const float* flow_or_null, const float* noise_or_null, uint8_t* dst_u8_hwc, int h, int w,
                void* stream) {
    const int rc = warp_check(src_u8_hwc, flow_or_null, noise_or_null, dst_u8_hwc, h, w);
    if (rc != VST_OK) return rc;
    const unsigned blocks = (unsigned)(((size_t)h * w + 255) / 256);
    warp_u8_kernel<<<blocks, 256, 0, (hipStream_t)stream>>>(src_u8_hwc, flow_or_null, noise_or_null, dst_u8_hwc, h, w);
    VST_RETURN_IF_LAUNCH_FAILED();
    return VST_OK;
}

int vst_warp_f32(const float* src_f32_planar, const float* flow_or_null, const float* noise_or_null, float* dst_f32_planar, int h,
                 int w, void* stream) {
    const int rc = warp_check(src_f32_planar, flow_or_null, noise_or_null, dst_f32_planar, h, w);
    if (rc != VST_OK) return rc;
    const unsigned blocks = (unsigned)(((size_t)h * w + 255) / 256);
    warp_f32_kernel<<<blocks, 256, 0, (hipStream_t)stream>>>(src_f32_planar, flow_or_null, noise_or_null, dst_f32_planar, h, w);
    VST_RETURN_IF_LAUNCH_FAILED();
    return VST_OK;
}

int vst_temporal_workspace_bytes(int h, int w, size_t* bytes) {
    if (!bytes) return VST_E_ARG;
    const int rc = frame_check(h, w);
    if (rc != VST_OK) return rc;
    *bytes = l1_blocks(h, w) * 3 * 8;
    return VST_OK;
}

int vst_temporal_l1_u8(const uint8_t* a_u8_hwc, const uint8_t* b_u8_hwc, const float* flow_or_null, int h, int w, double* loss3,
                       uint8_t* warped_or_null, void* ws, void* stream) {
    return temporal_l1<uint8_t, unsigned long long>(a_u8_hwc, b_u8_hwc, flow_or_null, h, w, loss3, warped_or_null, ws,
                                                    255.0 * (double)h * (double)w, (hipStream_t)stream);
}

int vst_temporal_l1_f32(const float* a_f32_planar, const float* b_f32_planar, const float* flow_or_null, int h, int w, double* loss3,
                        float* warped_or_null, void* ws, void* stream) {
    return temporal_l1<float, double>(a_f32_planar, b_f32_planar, flow_or_null, h, w, loss3, warped_or_null, ws,
                                      (double)h * (double)w, (hipStream_t)stream);
}

int vst_fake_flow_workspace_bytes(int h, int w, int gh, int gw, int ksize, size_t* bytes) {
    if (!bytes) return VST_E_ARG;
    const int rc = flow_check(h, w, gh, gw, ksize);
    if (rc != VST_OK) return rc;
    *bytes = ((size_t)w * gw + (size_t)h * gh + (size_t)2 * gh * w) * sizeof(double);
    return VST_OK;
}

int vst_fake_flow(const double* grid_f64, int gh, int gw, double shift_x, double shift_y, int ksize, float* flow_f32, int h, int w,
                  void* ws, void* stream) {
    if (!grid_f64 || !flow_f32 || !ws) return VST_E_ARG;
    const int rc = flow_check(h, w, gh, gw, ksize);
    if (rc != VST_OK) return rc;
    if (off_grid(grid_f64, 8) || off_grid(ws, 8) || off_grid(flow_f32, 4) || !(fabs(shift_x) < INFINITY) || !(fabs(shift_y) < INFINITY))
        return VST_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    double* bx = (double*)ws;
    double* by = bx + (size_t)w * gw;
    double* rows = by + (size_t)h * gh;
    const size_t n_tab = (size_t)w * gw + (size_t)h * gh, n_rows = (size_t)2 * gh * w;      // each at most 2^11 x 2^26: their grids stay below 2^31
    flow_tables_kernel<<<(unsigned)((n_tab + 255) / 256), 256, 0, st>>>(bx, h, w, gh, gw, ksize);
    VST_RETURN_IF_LAUNCH_FAILED();
    flow_rows_kernel<<<(unsigned)((n_rows + 255) / 256), 256, 0, st>>>(grid_f64, bx, rows, w, gh, gw);
    VST_RETURN_IF_LAUNCH_FAILED();
    flow_out_kernel<<<(unsigned)((size_t)h * ((w + 255) / 256)), 256, 0, st>>>(rows, by, flow_f32, h, w, gh, shift_x, shift_y);
    VST_RETURN_IF_LAUNCH_FAILED();
    return VST_OK;
}
