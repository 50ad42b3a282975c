// Frame resampling around the stylisation (vstnet.h, "Frame resampling"): Pillow's 8-bit bicubic resize, bit for bit, for the
// frames that enter the encoder (utils/utils.py:90-101 of the reference, called per frame at video_transfer.py:161), and the
// antialiased bicubic float resize to the writer size behind the decoder (video_transfer.py:210-212).  Both are separable and
// memory-bound: a horizontal pass, then a vertical pass, coefficient tables built on the host in double.
#include "common.h"
#include "deep_resize.h"
#include <math.h>

namespace {

// ------------------------------------------------------------------------------------------------ host: coefficient tables
// The bicubic kernel with a = -0.5 in the operation order both libraries use.  No contraction: an fma here would change the
// last bit of a coefficient and with it the 22-bit integer Pillow rounds it to.
#pragma clang fp contract(off)
double cubic(double x) {
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

// Pillow's triangle filter (Image.BILINEAR), support 1
double triangle(double x) {
    if (x < 0.0) x = -x;
    if (x < 1.0) return 1.0 - x;
    return 0.0;
}

// `support1` = the filter's support at scale 1: 2 for the bicubic tables, 1 for the bilinear one
int table_ksize(int in_size, int out_size, double support1 = 2.0) {
    double filterscale = (double)in_size / out_size;
    if (filterscale < 1.0) filterscale = 1.0;
    return (int)ceil(support1 * filterscale) * 2 + 1;
}

// one row of normalised double weights: k[0..n) (n <= ksize), returns n and the first input index.  `divide`: the filter
// argument as t / filterscale (the float resize's formula) instead of Pillow's t * (1 / filterscale)
int weights_row(int in_size, int out_size, int xx, bool divide, double* k, int* first, bool bilinear = false) {
    const double scale = (double)in_size / out_size;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = (bilinear ? 1.0 : 2.0) * filterscale;
    const double center = (xx + 0.5) * scale;
    const double ss = 1.0 / filterscale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    xmax -= xmin;
    double ww = 0.0;
    for (int x = 0; x < xmax; ++x) {
        const double t = x + xmin - center + 0.5;
        const double w = bilinear ? triangle(t * ss) : cubic(divide ? t / filterscale : t * ss);
        k[x] = w;
        ww += w;
    }
    for (int x = 0; x < xmax; ++x)
        if (ww != 0.0) k[x] /= ww;
    *first = xmin;
    return xmax;
}

int coeffs_check(int in_size, int out_size, const int* ksize) {
    if (!ksize || in_size <= 0 || out_size <= 0) return VST_E_ARG;
    if ((int64_t)in_size > (int64_t)VST_RESIZE_MAX_SHRINK * out_size) return VST_E_SHAPE;
    if (in_size > VST_MAX_FRAME_PIXELS || out_size > VST_MAX_FRAME_PIXELS) return VST_E_SHAPE;
    return VST_OK;
}

constexpr int MAX_KSIZE = 2 * 2 * VST_RESIZE_MAX_SHRINK + 1;
constexpr int PRECISION_BITS = 22;

// ------------------------------------------------------------------------------------------------ device
__device__ __forceinline__ unsigned clip8(int acc) {
    const int v = acc >> PRECISION_BITS;
    return (unsigned)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// what the element kinds differ in: Pillow's integers, fp32 fma, or - the deep resize - fp32 elements under double coefficients
// with fp64 accumulation and one rounding to fp32 per pass
struct U8Arith {
    typedef uint8_t elem;
    typedef int coef;
    typedef int acc;
    static __device__ __forceinline__ acc zero() { return 1 << (PRECISION_BITS - 1); }
    static __device__ __forceinline__ acc mad(acc a, elem v, coef c) { return a + (int)v * c; }
    static __device__ __forceinline__ elem done(acc a) { return (elem)clip8(a); }
};
struct F32Arith {
    typedef float elem;
    typedef float coef;
    typedef float acc;
    static __device__ __forceinline__ acc zero() { return 0.f; }
    static __device__ __forceinline__ acc mad(acc a, elem v, coef c) { return fmaf(v, c, a); }
    static __device__ __forceinline__ elem done(acc a) { return a; }
};
struct F64Arith {
    typedef float elem;
    typedef double coef;
    typedef double acc;
    static __device__ __forceinline__ acc zero() { return 0.0; }
    static __device__ __forceinline__ acc mad(acc a, elem v, coef c) { return fma((double)v, c, a); }
    static __device__ __forceinline__ elem done(acc a) { return (float)a; }
};

// Horizontal pass.  A workgroup owns PIX output columns of H_ROWS consecutive rows; a row holds C interleaved channels per
// pixel (uint8 RGB: 3; a float plane: 1) and thread t owns element t of the tile's PIX * C elements in every one of the rows,
// so a wave reads and writes consecutive elements.  The coefficient rows of the tile's columns are staged in LDS once and
// reused by the H_ROWS rows (row stride ksize is odd: neighbouring columns fall on different banks); the H_ROWS loads of a
// tap are independent.
constexpr int H_ROWS = 8;

template <typename A, int C, int PIX>
__global__ __launch_bounds__(PIX * C) void resize_h_kernel(const typename A::elem* __restrict__ src,
                                                           typename A::elem* __restrict__ dst, const int* __restrict__ table,
                                                           long rows, int Ws, int Wd, int ksize, int col_tiles) {
    extern __shared__ int lds[];
    int* lb = lds;                                              // [PIX][2]
    typename A::coef* lk = (typename A::coef*)(lds + 2 * PIX);  // [PIX][ksize]
    const int ct = blockIdx.x % col_tiles;
    const long y0 = (long)(blockIdx.x / col_tiles) * H_ROWS;
    const int x0 = ct * PIX;
    const int npix = Wd - x0 < PIX ? Wd - x0 : PIX;
    const int tid = threadIdx.x;
    for (int i = tid; i < 2 * npix; i += PIX * C) lb[i] = table[2 * (size_t)x0 + i];
    const typename A::coef* gk = (const typename A::coef*)(table + 2 * (size_t)Wd) + (size_t)x0 * ksize;
    for (int i = tid; i < npix * ksize; i += PIX * C) lk[i] = gk[i];
    __syncthreads();
    const int p = tid / C, c = tid - C * p;
    if (p >= npix) return;
    const int first = lb[2 * p], n = lb[2 * p + 1];
    const typename A::coef* k = lk + p * ksize;
    const size_t src_row = (size_t)Ws * C, dst_row = (size_t)Wd * C;
    const typename A::elem* s = src + (size_t)y0 * src_row + (size_t)first * C + c;
    typename A::elem* d = dst + (size_t)y0 * dst_row + (size_t)x0 * C + tid;
    typename A::acc acc[H_ROWS];
#pragma unroll
    for (int r = 0; r < H_ROWS; ++r) acc[r] = A::zero();
    if (y0 + H_ROWS <= rows) {
        for (int j = 0; j < n; ++j) {
            const typename A::coef cj = k[j];
#pragma unroll
            for (int r = 0; r < H_ROWS; ++r) acc[r] = A::mad(acc[r], s[r * src_row + (size_t)j * C], cj);
        }
#pragma unroll
        for (int r = 0; r < H_ROWS; ++r) d[r * dst_row] = A::done(acc[r]);
    } else {
        const int nr = (int)(rows - y0);
        for (int j = 0; j < n; ++j) {
            const typename A::coef cj = k[j];
#pragma unroll
            for (int r = 0; r < H_ROWS; ++r)
                if (r < nr) acc[r] = A::mad(acc[r], s[r * src_row + (size_t)j * C], cj);
        }
#pragma unroll
        for (int r = 0; r < H_ROWS; ++r)
            if (r < nr) d[r * dst_row] = A::done(acc[r]);
    }
}

// Vertical pass over uint8 rows of `rowbytes` bytes (channels do not matter here).  One workgroup per (output row, 256 * VEC
// bytes); the row's bounds and coefficients are the same for every lane (scalar loads); a thread owns VEC consecutive bytes
// and loads them as one 16-, 4- or 1-byte access (VEC = 16 / 4 need rowbytes % VEC == 0 and aligned bases).
template <int VEC>
__global__ __launch_bounds__(256) void resize_v_u8_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                          const int* __restrict__ table, size_t rowbytes, int Hd, int ksize,
                                                          int col_blocks) {
    const int y = blockIdx.x / col_blocks;
    const size_t b = ((size_t)(blockIdx.x % col_blocks) * 256 + threadIdx.x) * VEC;
    if (b >= rowbytes) return;
    const int first = table[2 * (size_t)y], n = table[2 * (size_t)y + 1];
    const int* __restrict__ k = table + 2 * (size_t)Hd + (size_t)y * ksize;
    const uint8_t* s = src + (size_t)first * rowbytes + b;
    int acc[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) acc[i] = 1 << (PRECISION_BITS - 1);
    for (int j = 0; j < n; ++j, s += rowbytes) {
        const int cj = k[j];
        if (VEC == 16) {
            const u32x4 v = *(const u32x4*)s;
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[i] += (int)((v[i >> 2] >> (8 * (i & 3))) & 255u) * cj;
        } else if (VEC == 4) {
            const unsigned v = *(const unsigned*)s;
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[i] += (int)((v >> (8 * i)) & 255u) * cj;
        } else {
            acc[0] += (int)s[0] * cj;
        }
    }
    uint8_t* d = dst + (size_t)y * rowbytes + b;
    if (VEC == 16) {
        u32x4 o;
#pragma unroll
        for (int q = 0; q < 4; ++q)
            o[q] = clip8(acc[4 * q]) | clip8(acc[4 * q + 1]) << 8 | clip8(acc[4 * q + 2]) << 16 | clip8(acc[4 * q + 3]) << 24;
        *(u32x4*)d = o;
    } else if (VEC == 4) {
        *(unsigned*)d = clip8(acc[0]) | clip8(acc[1]) << 8 | clip8(acc[2]) << 16 | clip8(acc[3]) << 24;
    } else {
        d[0] = (uint8_t)clip8(acc[0]);
    }
}

// Vertical pass over float planes [planes][Hs][W] -> [planes][Hd][W]: one thread per output value, workgroup = (plane, output
// row, 256 columns); the row's coefficients are uniform.
__global__ __launch_bounds__(256) void resize_v_f32_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                           const int* __restrict__ table, int Hs, int Hd, int W, int ksize,
                                                           int col_blocks) {
    const long row = blockIdx.x / col_blocks;                // plane * Hd + y
    const int x = (blockIdx.x % col_blocks) * 256 + threadIdx.x;
    if (x >= W) return;
    const long plane = row / Hd;
    const int y = (int)(row - plane * Hd);
    const int first = table[2 * (size_t)y], n = table[2 * (size_t)y + 1];
    const float* __restrict__ k = (const float*)(table + 2 * (size_t)Hd) + (size_t)y * ksize;
    const float* s = src + ((size_t)plane * Hs + first) * W + x;
    float acc = 0.f;
    for (int j = 0; j < n; ++j, s += W) acc = fmaf(s[0], k[j], acc);
    dst[(size_t)row * W + x] = acc;
}

// The same pass with the writer's epilogue: * 255, clamp, truncate, uint8 HWC.  A thread owns 4 consecutive bytes of the output
// row (each byte its own pixel and channel plane) and stores them as one dword where the address allows it.
__global__ __launch_bounds__(256) void resize_v_f32_u8_kernel(const float* __restrict__ src, uint8_t* __restrict__ dst,
                                                              const int* __restrict__ table, int Hs, int Hd, int W, int ksize,
                                                              int col_blocks) {
    const long row = blockIdx.x / col_blocks;                // image * Hd + y
    const int b0 = ((blockIdx.x % col_blocks) * 256 + threadIdx.x) * 4;
    const int rowbytes = 3 * W;
    if (b0 >= rowbytes) return;
    const long img = row / Hd;
    const int y = (int)(row - img * Hd);
    const int first = table[2 * (size_t)y], n = table[2 * (size_t)y + 1];
    const float* __restrict__ k = (const float*)(table + 2 * (size_t)Hd) + (size_t)y * ksize;
    const size_t plane = (size_t)Hs * W;
    const float* s[4];
    float acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        int b = b0 + i;
        b = b < rowbytes ? b : rowbytes - 1;                  // (the tail's spare lanes recompute the last byte; never stored)
        const int p = b / 3, c = b - 3 * p;
        s[i] = src + ((size_t)img * 3 + c) * plane + (size_t)first * W + p;
        acc[i] = 0.f;
    }
    for (int j = 0; j < n; ++j) {
        const float kj = k[j];
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] = fmaf(s[i][(size_t)j * W], kj, acc[i]);
    }
    unsigned q[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float v = acc[i] * 255.f;
        q[i] = (unsigned)(v < 0.f ? 0.f : (v > 255.f ? 255.f : v));       // clamp(0, 255) then truncation; NaN -> 0
    }
    uint8_t* d = dst + (size_t)row * rowbytes + b0;
    if (b0 + 4 <= rowbytes && (((size_t)d) & 3) == 0) *(unsigned*)d = q[0] | q[1] << 8 | q[2] << 16 | q[3] << 24;
    else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (b0 + i < rowbytes) d[i] = (uint8_t)q[i];
    }
}

// The deep resize's plain passes (vst_yuv16_img_resize_f32) over float planes [3][..][..] in F64Arith; a table's coefficients are
// doubles (two words each, the bounds' 2 * out words in front keep them on 8-byte addresses).  The horizontal pass is
// resize_h_kernel<F64Arith, 1, 64>.  Vertical: resize_v_f32_kernel's shape, a lane owning VEC = 4 consecutive columns as one
// 16-byte access where the row length and both bases allow it (else 1).  FINAL: the frame's last pass, with its epilogue
// (deep_resize.h: clamp, fp32 planes, the u8 twin if asked for) in the same launch.
template <bool FINAL, int VEC>
__global__ __launch_bounds__(256) void resize_v_f64_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                           uint8_t* __restrict__ dst_u8, const int* __restrict__ table, int Hs,
                                                           int Hd, int W, int ksize, int col_blocks) {
    const int row = blockIdx.x / col_blocks;                 // plane * Hd + y
    const int x = ((blockIdx.x % col_blocks) * blockDim.x + threadIdx.x) * VEC;      // (64 lanes per workgroup at VEC = 4)
    if (x >= W) return;
    const int plane = row / Hd, y = row - plane * Hd;
    const int first = table[2 * (size_t)y], n = table[2 * (size_t)y + 1];
    const double* __restrict__ k = (const double*)(table + 2 * (size_t)Hd) + (size_t)y * ksize;
    const float* s = src + ((size_t)plane * Hs + first) * W + x;
    F64Arith::acc acc[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) acc[i] = F64Arith::zero();
#pragma unroll 4
    for (int j = 0; j < n; ++j, s += W) {       // (the taps' loads are independent: four in flight per lane)
        const double kj = k[j];
        if (VEC == 4) {
            const float4 v = *reinterpret_cast<const float4*>(s);
            acc[0] = F64Arith::mad(acc[0], v.x, kj), acc[1] = F64Arith::mad(acc[1], v.y, kj);
            acc[2] = F64Arith::mad(acc[2], v.z, kj), acc[3] = F64Arith::mad(acc[3], v.w, kj);
        } else {
            acc[0] = F64Arith::mad(acc[0], s[0], kj);
        }
    }
    float* d = dst + (size_t)row * W + x;       // (final: the output planes [3][Hd][W] are laid out like any pass's)
    float o[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) o[i] = FINAL ? vst_deep_final_value(acc[i]) : F64Arith::done(acc[i]);
    if (VEC == 4) *reinterpret_cast<float4*>(d) = make_float4(o[0], o[1], o[2], o[3]);
    else d[0] = o[0];
    if (FINAL && dst_u8) {
#pragma unroll
        for (int i = 0; i < VEC; ++i) dst_u8[((size_t)y * W + x + i) * 3 + plane] = vst_deep_twin(o[i]);
    }
}

// A horizontal pass that is the frame's last (the last step changes the width alone): one thread per output value, workgroup =
// (plane row, 256 output columns), the weights from the table.  Small by then: the frame is at its stylised height.
__global__ __launch_bounds__(256) void resize_h_f64_final_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                                 uint8_t* __restrict__ dst_u8, const int* __restrict__ table, int H,
                                                                 int Ws, int Wd, int ksize, int col_blocks) {
    const int row = blockIdx.x / col_blocks;                 // plane * H + y
    const int x = (blockIdx.x % col_blocks) * 256 + threadIdx.x;
    if (x >= Wd) return;
    const int plane = row / H, y = row - plane * H;
    const int first = table[2 * (size_t)x], n = table[2 * (size_t)x + 1];
    const double* __restrict__ k = (const double*)(table + 2 * (size_t)Wd) + (size_t)x * ksize;
    const float* s = src + (size_t)row * Ws + first;
    F64Arith::acc acc = F64Arith::zero();
    for (int j = 0; j < n; ++j) acc = F64Arith::mad(acc, s[j], k[j]);
    vst_deep_final_store(dst, dst_u8, (size_t)H * Wd, Wd, plane, y, x, acc);
}

// ------------------------------------------------------------------------------------------------ host: checks and launches
int shape_check(int Hs, int Ws, int Hd, int Wd) {
    if (Hs <= 0 || Ws <= 0 || Hd <= 0 || Wd <= 0) return VST_E_ARG;
    if ((int64_t)Hs * Ws > VST_MAX_FRAME_PIXELS || (int64_t)Hd * Wd > VST_MAX_FRAME_PIXELS ||
        (int64_t)Hs * Wd > VST_MAX_FRAME_PIXELS)
        return VST_E_SHAPE;
    if ((int64_t)Hs > (int64_t)VST_RESIZE_MAX_SHRINK * Hd || (int64_t)Ws > (int64_t)VST_RESIZE_MAX_SHRINK * Wd) return VST_E_SHAPE;
    return VST_OK;
}

size_t table_words(int in_size, int out_size, double support1 = 2.0) {
    return (size_t)out_size * (2 + table_ksize(in_size, out_size, support1));
}

template <typename A, int C, int PIX>
int launch_h(const typename A::elem* src, typename A::elem* dst, const int* table, long rows, int Ws, int Wd, hipStream_t st,
             double support1 = 2.0) {
    const int ksize = table_ksize(Ws, Wd, support1);
    const int col_tiles = (Wd + PIX - 1) / PIX;
    const long blocks = (long)col_tiles * ((rows + H_ROWS - 1) / H_ROWS);
    if (blocks > 0x7fffffffL) return VST_E_SHAPE;
    const size_t lds = (size_t)PIX * (2 * sizeof(int) + ksize * sizeof(typename A::coef));
    resize_h_kernel<A, C, PIX><<<(unsigned)blocks, PIX * C, lds, st>>>(src, dst, table, rows, Ws, Wd, ksize, col_tiles);
    VST_RETURN_IF_LAUNCH_FAILED();
    return VST_OK;
}

// (`channels` bytes per pixel: 3 for an RGB frame, 1 for a grey map)
int launch_v_u8(const uint8_t* src, uint8_t* dst, const int* table, int Hs, int Hd, int W, hipStream_t st, int channels = 3,
                double support1 = 2.0) {
    const size_t rowbytes = (size_t)W * channels;
    const int ksize = table_ksize(Hs, Hd, support1);
    const size_t align = ((size_t)src) | ((size_t)dst) | rowbytes;
    const int vec = (align & 15) == 0 ? 16 : ((align & 3) == 0 ? 4 : 1);
    const int col_blocks = (int)((rowbytes / vec + 255) / 256);
    const long blocks = (long)col_blocks * Hd;
    if (blocks > 0x7fffffffL) return VST_E_SHAPE;
    if (vec == 16) resize_v_u8_kernel<16><<<(unsigned)blocks, 256, 0, st>>>(src, dst, table, rowbytes, Hd, ksize, col_blocks);
    else if (vec == 4) resize_v_u8_kernel<4><<<(unsigned)blocks, 256, 0, st>>>(src, dst, table, rowbytes, Hd, ksize, col_blocks);
    else resize_v_u8_kernel<1><<<(unsigned)blocks, 256, 0, st>>>(src, dst, table, rowbytes, Hd, ksize, col_blocks);
    VST_RETURN_IF_LAUNCH_FAILED();
    return VST_OK;
}

int resize_f32(const float* x, int B, int Hs, int Ws, float* dst_f32, uint8_t* dst_u8, int Hd, int Wd, const void* tables_dev,
               float* tmp, hipStream_t st) {
    if (!x || (!dst_f32 && !dst_u8) || !tables_dev || B <= 0) return VST_E_ARG;
    const int rc = shape_check(Hs, Ws, Hd, Wd);
    if (rc != VST_OK) return rc;
    const bool horizontal = Ws != Wd;
    if (horizontal && !tmp) return VST_E_ARG;
    const long planes = (long)B * 3;
    const int* th = (const int*)tables_dev;
    const int* tv = horizontal ? th + table_words(Ws, Wd) : th;
    const int ksize = table_ksize(Hs, Hd);
    const long rows = dst_u8 ? (long)B * Hd : planes * Hd;
    const int col_blocks = dst_u8 ? (3 * Wd + 1023) / 1024 : (Wd + 255) / 256;
    if (rows * col_blocks > 0x7fffffffL) return VST_E_SHAPE;
    if (horizontal) {
        const int r = launch_h<F32Arith, 1, 128>(x, tmp, th, planes * Hs, Ws, Wd, st);
        if (r != VST_OK) return r;
    }
    const float* vsrc = horizontal ? tmp : x;
    const unsigned blocks = (unsigned)(rows * col_blocks);
    if (dst_u8) resize_v_f32_u8_kernel<<<blocks, 256, 0, st>>>(vsrc, dst_u8, tv, Hs, Hd, Wd, ksize, col_blocks);
    else resize_v_f32_kernel<<<blocks, 256, 0, st>>>(vsrc, dst_f32, tv, Hs, Hd, Wd, ksize, col_blocks);
    VST_RETURN_IF_LAUNCH_FAILED();
    return VST_OK;
}

}  // namespace

namespace {

// Pillow's 8-bit table of either filter: normalised double weights rounded to 22-bit fixed point
int coeffs_u8(int in_size, int out_size, int* ksize, int* bounds, int* kk, bool bilinear) {
    const int rc = coeffs_check(in_size, out_size, ksize);
    if (rc != VST_OK) return rc;
    const int ks = *ksize = table_ksize(in_size, out_size, bilinear ? 1.0 : 2.0);
    if (!bounds || !kk) return VST_OK;
    double k[MAX_KSIZE];
    for (int xx = 0; xx < out_size; ++xx) {
        int first = 0;
        const int n = weights_row(in_size, out_size, xx, false, k, &first, bilinear);
        bounds[2 * (size_t)xx] = first;
        bounds[2 * (size_t)xx + 1] = n;
        int* row = kk + (size_t)xx * ks;
        for (int x = 0; x < ks; ++x) {
            const double v = x < n ? k[x] : 0.0;
            row[x] = v < 0 ? (int)(-0.5 + v * (1 << PRECISION_BITS)) : (int)(0.5 + v * (1 << PRECISION_BITS));
        }
    }
    return VST_OK;
}

}  // namespace

int vst_resize_coeffs_u8(int in_size, int out_size, int* ksize, int* bounds, int* kk) {
    return coeffs_u8(in_size, out_size, ksize, bounds, kk, false);
}

int vst_resize_coeffs_u8_bilinear(int in_size, int out_size, int* ksize, int* bounds, int* kk) {
    return coeffs_u8(in_size, out_size, ksize, bounds, kk, true);
}

int vst_resize_coeffs_f32(int in_size, int out_size, int* ksize, int* xmin, float* w) {
    const int rc = coeffs_check(in_size, out_size, ksize);
    if (rc != VST_OK) return rc;
    const int ks = *ksize = table_ksize(in_size, out_size);
    if (!xmin || !w) return VST_OK;
    double k[MAX_KSIZE];
    for (int xx = 0; xx < out_size; ++xx) {
        int first = 0;
        const int n = weights_row(in_size, out_size, xx, true, k, &first);
        xmin[2 * (size_t)xx] = first;
        xmin[2 * (size_t)xx + 1] = n;
        float* row = w + (size_t)xx * ks;
        for (int x = 0; x < ks; ++x) row[x] = x < n ? (float)k[x] : 0.f;
    }
    return VST_OK;
}

int vst_resize_u8(const uint8_t* src_hwc, int Hs, int Ws, uint8_t* dst_hwc, int Hd, int Wd, const int* tables_dev, uint8_t* tmp,
                  void* stream) {
    if (!src_hwc || !dst_hwc) return VST_E_ARG;
    const int rc = shape_check(Hs, Ws, Hd, Wd);
    if (rc != VST_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    const bool horizontal = Ws != Wd, vertical = Hs != Hd;
    if ((horizontal || vertical) && !tables_dev) return VST_E_ARG;
    if (horizontal && vertical && !tmp) return VST_E_ARG;
    if (!horizontal && !vertical) return (int)hipMemcpyAsync(dst_hwc, src_hwc, (size_t)Hs * Ws * 3, hipMemcpyDeviceToDevice, st);
    const int* tv = horizontal ? tables_dev + table_words(Ws, Wd) : tables_dev;
    const uint8_t* vsrc = src_hwc;
    if (horizontal) {
        uint8_t* hdst = vertical ? tmp : dst_hwc;
        const int r = launch_h<U8Arith, 3, 64>(src_hwc, hdst, tables_dev, Hs, Ws, Wd, st);
        if (r != VST_OK) return r;
        vsrc = hdst;
    }
    return vertical ? launch_v_u8(vsrc, dst_hwc, tv, Hs, Hd, Wd, st) : VST_OK;
}

// Image.resize((Wd, Hd), BILINEAR) of an "L" image: vst_resize_u8's passes on one channel with the bilinear tables
int vst_resize_grey_u8(const uint8_t* src, int Hs, int Ws, uint8_t* dst, int Hd, int Wd, const int* tables_dev, uint8_t* tmp,
                       void* stream) {
    if (!src || !dst) return VST_E_ARG;
    const int rc = shape_check(Hs, Ws, Hd, Wd);
    if (rc != VST_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    const bool horizontal = Ws != Wd, vertical = Hs != Hd;
    if ((horizontal || vertical) && !tables_dev) return VST_E_ARG;
    if (horizontal && vertical && !tmp) return VST_E_ARG;
    if (!horizontal && !vertical) return (int)hipMemcpyAsync(dst, src, (size_t)Hs * Ws, hipMemcpyDeviceToDevice, st);
    const int* tv = horizontal ? tables_dev + table_words(Ws, Wd, 1.0) : tables_dev;
    const uint8_t* vsrc = src;
    if (horizontal) {
        uint8_t* hdst = vertical ? tmp : dst;
        const int r = launch_h<U8Arith, 1, 128>(src, hdst, tables_dev, Hs, Ws, Wd, st, 1.0);
        if (r != VST_OK) return r;
        vsrc = hdst;
    }
    return vertical ? launch_v_u8(vsrc, dst, tv, Hs, Hd, Wd, st, 1, 1.0) : VST_OK;
}

int vst_resize_f32(const float* x_planar, int B, int Hs, int Ws, float* dst_planar, int Hd, int Wd, const void* tables_dev,
                   float* tmp, void* stream) {
    if (!dst_planar) return VST_E_ARG;
    return resize_f32(x_planar, B, Hs, Ws, dst_planar, nullptr, Hd, Wd, tables_dev, tmp, (hipStream_t)stream);
}

int vst_resize_f32_to_u8(const float* x_planar, int B, int Hs, int Ws, uint8_t* dst_hwc, int Hd, int Wd, const void* tables_dev,
                         float* tmp, void* stream) {
    if (!dst_hwc) return VST_E_ARG;
    return resize_f32(x_planar, B, Hs, Ws, nullptr, dst_hwc, Hd, Wd, tables_dev, tmp, (hipStream_t)stream);
}

int vst_resize_coeffs_f64(int in_size, int out_size, int* ksize, int* bounds, double* w) {
    const int rc = coeffs_check(in_size, out_size, ksize);
    if (rc != VST_OK) return rc;
    const int ks = *ksize = table_ksize(in_size, out_size);
    if (!bounds || !w) return VST_OK;
    double k[MAX_KSIZE];
    for (int xx = 0; xx < out_size; ++xx) {
        int first = 0;
        const int n = weights_row(in_size, out_size, xx, false, k, &first);
        bounds[2 * (size_t)xx] = first;
        bounds[2 * (size_t)xx + 1] = n;
        double* row = w + (size_t)xx * ks;
        for (int x = 0; x < ks; ++x) row[x] = x < n ? k[x] : 0.0;
    }
    return VST_OK;
}

namespace {

// The passes of a deep resize, in order.  An intermediate - the source-size RGB where the first pass is vertical, then every pass's
// output but the last - lives in the workspace: intermediate i in half i & 1, each half as large as its largest tenant.
struct DeepPass {
    bool horizontal;
    int in, out, other;         // the axis' sizes, and the other axis' (rows of a horizontal pass, columns of a vertical one)
    size_t table_word;          // where the pass's table starts in tables_dev
};
constexpr int DEEP_MAX_STEPS = 4;
struct DeepPlan {
    int n = 0, W = 0, H = 0;    // passes; the final size
    DeepPass pass[2 * DEEP_MAX_STEPS];
    bool unfused = false;       // the first pass is vertical: the frame is converted at the source size first
    size_t half[2] = {0, 0};    // floats
};

int deep_plan(int Hs, int Ws, int nsteps, const int* steps_wh, DeepPlan& p) {
    if (Hs < 1 || Ws < 1 || nsteps < 0 || nsteps > DEEP_MAX_STEPS || (nsteps > 0 && !steps_wh)) return VST_E_ARG;
    if ((int64_t)Hs * Ws > VST_MAX_FRAME_PIXELS) return VST_E_SHAPE;
    int w = Ws, h = Hs;
    size_t word = 0;
    for (int s = 0; s < nsteps; ++s) {
        const int tw = steps_wh[2 * s], th = steps_wh[2 * s + 1];
        if (tw < 1 || th < 1) return VST_E_ARG;
        if (tw > w || th > h) return VST_E_SHAPE;                                   // sizes only shrink
        if ((int64_t)w > (int64_t)VST_RESIZE_MAX_SHRINK * tw || (int64_t)h > (int64_t)VST_RESIZE_MAX_SHRINK * th) return VST_E_SHAPE;
        if (tw != w) {
            p.pass[p.n++] = DeepPass{true, w, tw, h, word};
            word += (size_t)tw * (2 + 2 * table_ksize(w, tw));
            w = tw;
        }
        if (th != h) {
            p.pass[p.n++] = DeepPass{false, h, th, w, word};
            word += (size_t)th * (2 + 2 * table_ksize(h, th));
            h = th;
        }
    }
    p.W = w, p.H = h;
    p.unfused = p.n > 0 && !p.pass[0].horizontal;
    int idx = 0;
    if (p.unfused) p.half[idx++ & 1] = (size_t)3 * Hs * Ws;
    for (int i = 0; i + 1 < p.n; ++i, ++idx) {
        const DeepPass& q = p.pass[i];
        const size_t floats = (size_t)3 * q.out * q.other;
        if (floats > p.half[idx & 1]) p.half[idx & 1] = floats;
    }
    if (p.half[1] > 0) p.half[0] = (p.half[0] + 63) / 64 * 64;      // (the second half starts on a 256-byte address)
    return VST_OK;
}

}  // namespace

int vst_yuv16_img_resize_workspace_bytes(int Hs, int Ws, int nsteps, const int* steps_wh, size_t* bytes) {
    if (!bytes) return VST_E_ARG;
    DeepPlan p;
    const int rc = deep_plan(Hs, Ws, nsteps, steps_wh, p);
    if (rc != VST_OK) return rc;
    *bytes = (p.half[0] + p.half[1]) * sizeof(float);
    return VST_OK;
}

int vst_yuv16_img_resize_f32(const uint16_t* y, const uint16_t* u, const uint16_t* v, int Hs, int Ws, int depth, int layout,
                             int matrix, int range, int nsteps, const int* steps_wh, const void* tables_dev, float* work,
                             float* out_f32, uint8_t* out_u8, void* stream) {
    if (!out_f32) return VST_E_ARG;
    int rc = vst_deep_yuv_check(y, u, v, Hs, Ws, depth, layout, matrix, range);
    if (rc != VST_OK) return rc;
    DeepPlan p;
    rc = deep_plan(Hs, Ws, nsteps, steps_wh, p);
    if (rc != VST_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (p.n == 0) return vst_yuv16_to_rgb_f32(y, u, v, Hs, Ws, depth, layout, matrix, range, out_f32, out_u8, stream);
    if (!tables_dev || ((p.half[0] + p.half[1]) > 0 && !work)) return VST_E_ARG;
    if ((((uintptr_t)tables_dev) & 7) != 0 || (((uintptr_t)work) & 3) != 0) return VST_E_ARG;   // (a table's weights are doubles)
    for (int i = 0; i < p.n; ++i) {             // every launch's grid, before the first launch
        const DeepPass& q = p.pass[i];
        const int64_t blocks = q.horizontal ? (int64_t)((q.out + 63) / 64) * (((int64_t)3 * q.other + H_ROWS - 1) / H_ROWS) +
                                                  (int64_t)((q.out + 255) / 256) * 3 * q.other
                                            : (int64_t)((q.other + 255) / 256) * 3 * q.out;
        if (blocks > 0x7fffffffLL) return VST_E_SHAPE;
    }
    const int* tables = (const int*)tables_dev;
    float* half[2] = {work, work + p.half[0]};
    int idx = 0;
    const float* cur = nullptr;
    int first = 0;
    if (p.unfused) {
        rc = vst_yuv16_to_rgb_f32(y, u, v, Hs, Ws, depth, layout, matrix, range, half[0], nullptr, stream);
        if (rc != VST_OK) return rc;
        cur = half[0], idx = 1;
    } else {
        const DeepPass& q = p.pass[0];
        const bool final = p.n == 1;
        float* dst = final ? out_f32 : half[0];
        rc = vst_deep_resize_h_fused(y, u, v, Hs, Ws, depth, layout, matrix, range, tables + q.table_word, q.out,
                                     table_ksize(q.in, q.out), dst, final ? out_u8 : nullptr, final ? 1 : 0, st);
        if (rc != VST_OK) return rc;
        cur = dst, idx = 1, first = 1;
    }
    for (int i = first; i < p.n; ++i, ++idx) {
        const DeepPass& q = p.pass[i];
        const bool final = i == p.n - 1;
        float* dst = final ? out_f32 : half[idx & 1];
        const int* table = tables + q.table_word;
        const int ksize = table_ksize(q.in, q.out);
        if (q.horizontal && !final) {
            rc = launch_h<F64Arith, 1, 64>(cur, dst, table, (long)3 * q.other, q.in, q.out, st);
            if (rc != VST_OK) return rc;
        } else if (q.horizontal) {
            const int col_blocks = (q.out + 255) / 256;
            resize_h_f64_final_kernel<<<(unsigned)(col_blocks * 3 * q.other), 256, 0, st>>>(cur, dst, out_u8, table, q.other, q.in,
                                                                                           q.out, ksize, col_blocks);
            VST_RETURN_IF_LAUNCH_FAILED();
        } else {
            const bool vec4 = (q.other & 3) == 0 && ((((uintptr_t)cur) | ((uintptr_t)dst)) & 15) == 0;
            // a workgroup is one output row's 256 columns either way: 64 lanes of 4 columns (a 1280-wide row is 5 full workgroups:
            // no idle lanes behind a ragged end), or 256 lanes of one
            const int threads = vec4 ? 64 : 256;
            const int col_blocks = (q.other + 255) / 256;
            const unsigned blocks = (unsigned)(col_blocks * 3 * q.out);
            uint8_t* twin = final ? out_u8 : nullptr;
            if (final && vec4) resize_v_f64_kernel<true, 4><<<blocks, threads, 0, st>>>(cur, dst, twin, table, q.in, q.out, q.other, ksize, col_blocks);
            else if (final) resize_v_f64_kernel<true, 1><<<blocks, threads, 0, st>>>(cur, dst, twin, table, q.in, q.out, q.other, ksize, col_blocks);
            else if (vec4) resize_v_f64_kernel<false, 4><<<blocks, threads, 0, st>>>(cur, dst, twin, table, q.in, q.out, q.other, ksize, col_blocks);
            else resize_v_f64_kernel<false, 1><<<blocks, threads, 0, st>>>(cur, dst, twin, table, q.in, q.out, q.other, ksize, col_blocks);
            VST_RETURN_IF_LAUNCH_FAILED();
        }
        cur = dst;
    }
    return VST_OK;
}
