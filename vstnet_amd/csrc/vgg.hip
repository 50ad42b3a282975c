// Style loss on gfx950 ("Style loss"): the reference's VGG-19 encoder up to relu4_1 (models/VGG.py,
// build_vgg: Sequential indices 0 .. 29), the per-channel mean / std records of its four taps, and the two numbers the reference
// trains on: loss_s = sum_l mse(mean_a, mean_b) + mse(std_a, std_b) and loss_c = mse(relu4_1(a), relu4_1(b)).
//
// Maps are token-major fp32 [H*W][C], the segmenter's layout, so a 3 x 3 conv under ReflectionPad2d(1) is the segmenter's GEMM
// out[M][N] = A[M][K] . W[N][K]^T + bias with M = H W, N = Cout, K = 9 Cin in K order (ky, kx, c), and row m = (y, x) of A
// is nine contiguous runs of Cin floats of the input map.  vgg_conv_kernel IS seg_gemm_kernel (csrc/segformer.hip) with that
// gather as its A-loader: same tile, same three-way bf16 split, same six products into big0 / big1 / small, same order of additions
// in the epilogue - so it returns ReLU(vst_seg_gemm(col, W, bias)) bit for bit and inherits that kernel's fp64 tests, while the
// [M][9 Cin] column matrix (9 x the input map: 4.8 GB for conv1_2 at 1080p) never exists.  Everything else here is a copy, a
// maximum or an fp64 reduction in a fixed order (no atomics: the same input gives the same bits on every run).
#include "common.h"
#include <algorithm>
#include <map>
#include <string>
#include <vector>

namespace {

constexpr int64_t VGG_MAX_PIXELS = (int64_t)1 << 24;          // whole-frame limit of a features run (4096 x 4096)
constexpr int64_t VGG_OP_MAX_FLOATS = (int64_t)1 << 30;      // per operand of a kernel-level call
constexpr int VGG_LEVELS = 4;
constexpr int VGG_C[VGG_LEVELS] = {64, 128, 256, 512};
static_assert(2 * (VGG_C[0] + VGG_C[1] + VGG_C[2] + VGG_C[3]) == VST_VGG_RECORD_DOUBLES, "vstnet.h: VST_VGG_RECORD_DOUBLES");

// ------------------------------------------------------------------------------------------------------------- input
// x = v / 255 (u8) or v (f32), then the reference's 1 x 1 conv in a fixed order with every product and sum rounded to fp32
// (contraction into FMAs is off): ((a0 x0 + a1 x1) + a2 x2) + b.  Channel 3 of the output is 0.
__device__ __forceinline__ float vgg_dot3(const float* a, const float (&x)[3], float b) {
#pragma clang fp contract(off)
    return ((a[0] * x[0] + a[1] * x[1]) + a[2] * x[2]) + b;
}

template <bool U8>
__global__ void vgg_input_kernel(const void* __restrict__ frame, const float* __restrict__ w, const float* __restrict__ bias,
                                 float4* __restrict__ out, int H, int W) {
    const size_t n = (size_t)H * W;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float x[3];
    if (U8) {
        const uint8_t* p = static_cast<const uint8_t*>(frame) + i * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) x[c] = (float)p[c] / 255.f;
    } else {
        const float* p = static_cast<const float*>(frame);
#pragma unroll
        for (int c = 0; c < 3; ++c) x[c] = p[(size_t)c * n + i];
    }
    float y[3];
#pragma unroll
    for (int o = 0; o < 3; ++o) y[o] = vgg_dot3(w + 3 * o, x, bias[o]);
    out[i] = make_float4(y[0], y[1], y[2], 0.f);
}

// -------------------------------------------------------------------------------------------------------------- conv
// seg_gemm_kernel's geometry: 64 x 64 output tile per workgroup, 4 waves, wave w owns rows 16w .. 16w+15 and all 64 columns.
constexpr int G_TILE = 64;
constexpr int G_K = 32;
constexpr int G_LD = 40;        // bf16 per LDS row: 32 + 8 of padding

// ReflectionPad2d(1): v in -1 .. n with n >= 2
__device__ __forceinline__ int vgg_reflect(int v, int n) { return v < 0 ? -v : (v >= n ? 2 * n - 2 - v : v); }

__global__ __launch_bounds__(256) void vgg_conv_kernel(const float* __restrict__ in, const float* __restrict__ Wt,
                                                       const float* __restrict__ bias, float* __restrict__ out, int H, int W,
                                                       int Cin, int N) {
    __shared__ __attribute__((aligned(16))) __bf16 s_hi[2][G_TILE * G_LD];
    __shared__ __attribute__((aligned(16))) __bf16 s_md[2][G_TILE * G_LD];
    __shared__ __attribute__((aligned(16))) __bf16 s_lo[2][G_TILE * G_LD];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int m0 = blockIdx.x * G_TILE, n0 = blockIdx.y * G_TILE;
    const int M = H * W, K = 9 * Cin;          // K % 4 == 0: a group of 4 consecutive k is inside K or past it, and inside one tap
    // the two rows of A this thread stages (tile rows tid >> 3 and 32 + (tid >> 3)): their pixel, or y = -1 past M
    int py[2], px[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int r = m0 + (tid >> 3) + 32 * i;
        py[i] = -1; px[i] = 0;
        if (r < M) { py[i] = r / W; px[i] = r - py[i] * W; }
    }
    f32x4 big0[4], big1[4], small[4];
#pragma unroll
    for (int n = 0; n < 4; ++n) big0[n] = big1[n] = small[n] = f32x4{0.f, 0.f, 0.f, 0.f};

    auto k_step = [&](int k0, f32x4 (&big)[4]) {
        // stage 64 x 32 of A (gathered) and of W: 2 x 512 groups of 4 consecutive k; rows past M / N and k past K are zeros
        const int kq = (tid & 7) * 4;
        const int k = k0 + kq;
        int ky = 0, kx = 0, c = 0;
        if (k < K) {
            const int tap = k / Cin;
            c = k - tap * Cin;
            ky = tap / 3;
            kx = tap - 3 * ky;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int mat = i >> 1;
            const int row = (tid >> 3) + 32 * (i & 1);
            float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
            if (k < K) {
                if (mat == 0) {
                    if (py[i & 1] >= 0) {
                        const int ry = vgg_reflect(py[i & 1] + ky - 1, H), rx = vgg_reflect(px[i & 1] + kx - 1, W);
                        t = *reinterpret_cast<const float4*>(in + ((size_t)ry * W + rx) * Cin + c);
                    }
                } else if (n0 + row < N) {
                    t = *reinterpret_cast<const float4*>(Wt + (size_t)(n0 + row) * K + k);
                }
            }
            const float v[4] = {t.x, t.y, t.z, t.w};
            bf16x4 h, m, l;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                h[j] = (__bf16)v[j];
                const float r = v[j] - (float)h[j];          // exact in fp32
                m[j] = (__bf16)r;
                l[j] = (__bf16)(r - (float)m[j]);
            }
            *reinterpret_cast<bf16x4*>(&s_hi[mat][row * G_LD + kq]) = h;
            *reinterpret_cast<bf16x4*>(&s_md[mat][row * G_LD + kq]) = m;
            *reinterpret_cast<bf16x4*>(&s_lo[mat][row * G_LD + kq]) = l;
        }
        __syncthreads();
        const int a_off = (wave * 16 + (lane & 15)) * G_LD + (lane >> 4) * 8;
        const bf16x8 ah = *reinterpret_cast<const bf16x8*>(&s_hi[0][a_off]);
        const bf16x8 am = *reinterpret_cast<const bf16x8*>(&s_md[0][a_off]);
        const bf16x8 al = *reinterpret_cast<const bf16x8*>(&s_lo[0][a_off]);
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            const int w_off = (n * 16 + (lane & 15)) * G_LD + (lane >> 4) * 8;
            const bf16x8 wh = *reinterpret_cast<const bf16x8*>(&s_hi[1][w_off]);
            const bf16x8 wm = *reinterpret_cast<const bf16x8*>(&s_md[1][w_off]);
            const bf16x8 wl = *reinterpret_cast<const bf16x8*>(&s_lo[1][w_off]);
            small[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, wh, small[n], 0, 0, 0);      // smallest terms first
            small[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, wl, small[n], 0, 0, 0);
            small[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(am, wm, small[n], 0, 0, 0);
            small[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(am, wh, small[n], 0, 0, 0);
            small[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, wm, small[n], 0, 0, 0);
            big[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, wh, big[n], 0, 0, 0);
        }
        __syncthreads();
    };
    for (int k0 = 0; k0 < K; k0 += 2 * G_K) {          // (K and the trip count are uniform over the workgroup)
        k_step(k0, big0);
        if (k0 + G_K < K) k_step(k0 + G_K, big1);
    }
    // D: column = lane & 15, row = 4 (lane >> 4) + register
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        const int col = n0 + n * 16 + (lane & 15);
        if (col >= N) continue;
        const float b = bias[col];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = m0 + wave * 16 + (lane >> 4) * 4 + r;
            if (row >= M) continue;
            const float v = ((big0[n][r] + big1[n][r]) + small[n][r]) + b;
            out[(size_t)row * N + col] = fmaxf(v, 0.f);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------- max-pool
// 2 x 2 / stride 2 with ceil_mode: the last window of an odd edge is partial.  One thread per float4 of the output; the
// running maximum is replaced only by a strictly larger value, in (dy, dx) order, as torch's max_pool2d does.
__global__ void vgg_maxpool_kernel(const float* __restrict__ in, float* __restrict__ out, int H, int W, int C, int Ho, int Wo) {
    const int c4n = C >> 2;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)Ho * Wo * c4n) return;
    const int c4 = (int)(idx % c4n);
    const size_t cell = idx / c4n;
    const int oy = (int)(cell / Wo), ox = (int)(cell % Wo);
    float4 m = *reinterpret_cast<const float4*>(in + ((size_t)(2 * oy) * W + 2 * ox) * C + c4 * 4);
#pragma unroll
    for (int d = 1; d < 4; ++d) {
        const int iy = 2 * oy + (d >> 1), ix = 2 * ox + (d & 1);
        if (iy >= H || ix >= W) continue;
        const float4 v = *reinterpret_cast<const float4*>(in + ((size_t)iy * W + ix) * C + c4 * 4);
        m.x = v.x > m.x ? v.x : m.x; m.y = v.y > m.y ? v.y : m.y;
        m.z = v.z > m.z ? v.z : m.z; m.w = v.w > m.w ? v.w : m.w;
    }
    *reinterpret_cast<float4*>(out + cell * C + c4 * 4) = m;
}

// ---------------------------------------------------------------------------------------------------------- mean / std
// Per channel over the n rows of a map, in fp64, two passes: the rows are cut into `nch` chunks; a workgroup of 4 x 64 threads
// sums one chunk of 64 channels (thread (j, c): rows j, j + 4, ... of the chunk, then the four j in order), and one thread per
// channel adds the chunks in order.  SQ = 0: sum x; SQ = 1: sum (x - mean)^2 with the mean the first pass left in rec[0][c].
constexpr int ST_MAX_CHUNKS = 1024;
constexpr int ST_CHUNK_MIN_ROWS = 64;

inline int vgg_stat_chunks(size_t n) {
    return (int)std::min<size_t>(ST_MAX_CHUNKS, (n + ST_CHUNK_MIN_ROWS - 1) / ST_CHUNK_MIN_ROWS);
}

template <int SQ>
__global__ __launch_bounds__(256) void vgg_stat_partial_kernel(const float* __restrict__ in, size_t n, int C, size_t rows_per_chunk,
                                                               const double* __restrict__ rec, double* __restrict__ part) {
    __shared__ double s[4][64];
    const int cl = threadIdx.x & 63, j = threadIdx.x >> 6;
    const int c = blockIdx.y * 64 + cl;
    const size_t r0 = (size_t)blockIdx.x * rows_per_chunk, r1 = r0 + rows_per_chunk < n ? r0 + rows_per_chunk : n;
    double acc = 0.0;
    if (c < C) {
        const double mean = SQ ? rec[c] : 0.0;
#pragma unroll 4
        for (size_t r = r0 + j; r < r1; r += 4) {
            const double d = (double)in[r * C + c] - mean;
            acc += SQ ? d * d : d;
        }
    }
    s[j][cl] = acc;
    __syncthreads();
    if (j == 0 && c < C) part[(size_t)blockIdx.x * C + c] = ((s[0][cl] + s[1][cl]) + s[2][cl]) + s[3][cl];
}

// SQ = 0: rec[0][c] = sum / n;  SQ = 1: rec[1][c] = sqrt(sum / (n - 1) + eps)   (torch's var is unbiased)
template <int SQ>
__global__ void vgg_stat_final_kernel(const double* __restrict__ part, int nch, size_t n, int C, double eps, double* __restrict__ rec) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    double acc = 0.0;
    for (int k = 0; k < nch; ++k) acc += part[(size_t)k * C + c];
    if (SQ) rec[C + c] = sqrt(acc / (double)(n - 1) + eps);
    else rec[c] = acc / (double)n;
}

// ---------------------------------------------------------------------------------------------------------------- MSE
// fixed-order fp64 sum of one workgroup's 256 values (a tree over LDS); the result is in s[0]
__device__ __forceinline__ void vgg_block_sum(double* s, double v) {
    s[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) s[threadIdx.x] += s[threadIdx.x + o];
        __syncthreads();
    }
}

constexpr int MSE_MAX_BLOCKS = VST_VGG_MSE_WS_BYTES / 8;

__global__ __launch_bounds__(256) void vgg_mse_partial_kernel(const float* __restrict__ a, const float* __restrict__ b, size_t count,
                                                              double* __restrict__ part) {
    __shared__ double s[256];
    double acc = 0.0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (size_t)gridDim.x * 256) {
        const double d = (double)a[i] - (double)b[i];
        acc += d * d;
    }
    vgg_block_sum(s, acc);
    if (threadIdx.x == 0) part[blockIdx.x] = s[0];
}

__global__ __launch_bounds__(256) void vgg_mse_final_kernel(const double* __restrict__ part, int nparts, size_t count,
                                                            double* __restrict__ out) {
    __shared__ double s[256];
    double acc = 0.0;
    for (int i = threadIdx.x; i < nparts; i += 256) acc += part[i];
    vgg_block_sum(s, acc);
    if (threadIdx.x == 0) out[0] = s[0] / (double)count;
}

// ---------------------------------------------------------------------------------------------------------- style loss
// one workgroup: per level mse(mean_a, mean_b) + mse(std_a, std_b), the levels added in order
__global__ __launch_bounds__(256) void vgg_style_loss_kernel(const double* __restrict__ ra, const double* __restrict__ rb,
                                                             double* __restrict__ out) {
    __shared__ double s[256];
    double total = 0.0;
    size_t at = 0;
    for (int l = 0; l < VGG_LEVELS; ++l) {
        const int C = VGG_C[l];
        double level = 0.0;
        for (int part = 0; part < 2; ++part) {
            double acc = 0.0;
            for (int c = threadIdx.x; c < C; c += 256) {
                const double d = ra[at + c] - rb[at + c];
                acc += d * d;
            }
            vgg_block_sum(s, acc);
            level += s[0] / (double)C;
            __syncthreads();
            at += C;
        }
        total += level;
    }
    if (threadIdx.x == 0) out[0] = total;
}

// ------------------------------------------------------------------------------------------------------------ launchers
inline unsigned blocks_for(size_t n, int per) { return (unsigned)((n + per - 1) / per); }
inline bool vgg_f4(const void* p) { return p && ((uintptr_t)p & 15) == 0; }
inline bool vgg_f8(const void* p) { return p && ((uintptr_t)p & 7) == 0; }
inline bool vgg_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + nb && b0 < a0 + na;
}

int vgg_input(const void* frame, bool u8, const float* w, const float* b, float* out, int H, int W, hipStream_t st) {
    const unsigned g = blocks_for((size_t)H * W, 256);
    if (u8) vgg_input_kernel<true><<<g, 256, 0, st>>>(frame, w, b, reinterpret_cast<float4*>(out), H, W);
    else vgg_input_kernel<false><<<g, 256, 0, st>>>(frame, w, b, reinterpret_cast<float4*>(out), H, W);
    VST_RETURN_IF_LAUNCH_FAILED();
    return VST_OK;
}
int vgg_conv(const float* in, const float* w, const float* bias, float* out, int H, int W, int Cin, int Cout, hipStream_t st) {
    dim3 grid(blocks_for((size_t)H * W, G_TILE), blocks_for((size_t)Cout, G_TILE));
    vgg_conv_kernel<<<grid, 256, 0, st>>>(in, w, bias, out, H, W, Cin, Cout);
    VST_RETURN_IF_LAUNCH_FAILED();
    return VST_OK;
}
int vgg_maxpool(const float* in, float* out, int H, int W, int C, hipStream_t st) {
    const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
    vgg_maxpool_kernel<<<blocks_for((size_t)Ho * Wo * (C / 4), 256), 256, 0, st>>>(in, out, H, W, C, Ho, Wo);
    VST_RETURN_IF_LAUNCH_FAILED();
    return VST_OK;
}
size_t vgg_mean_std_bytes(size_t n, int C) { return (size_t)vgg_stat_chunks(n) * C * sizeof(double); }
int vgg_mean_std(const float* in, size_t n, int C, double eps, double* rec, double* ws, hipStream_t st) {
    const int nch = vgg_stat_chunks(n);
    const size_t rows = (n + nch - 1) / nch;
    const dim3 grid(nch, blocks_for((size_t)C, 64));
    vgg_stat_partial_kernel<0><<<grid, 256, 0, st>>>(in, n, C, rows, rec, ws);
    vgg_stat_final_kernel<0><<<blocks_for((size_t)C, 64), 64, 0, st>>>(ws, nch, n, C, eps, rec);
    vgg_stat_partial_kernel<1><<<grid, 256, 0, st>>>(in, n, C, rows, rec, ws);
    vgg_stat_final_kernel<1><<<blocks_for((size_t)C, 64), 64, 0, st>>>(ws, nch, n, C, eps, rec);
    VST_RETURN_IF_LAUNCH_FAILED();
    return VST_OK;
}
int vgg_mse(const float* a, const float* b, size_t count, double* out, double* ws, hipStream_t st) {
    const int nb = (int)std::min<size_t>(MSE_MAX_BLOCKS, (count + 1023) / 1024);
    vgg_mse_partial_kernel<<<nb, 256, 0, st>>>(a, b, count, ws);
    vgg_mse_final_kernel<<<1, 256, 0, st>>>(ws, nb, count, out);
    VST_RETURN_IF_LAUNCH_FAILED();
    return VST_OK;
}

// ----------------------------------------------------------------------------------------------------------------- plan
struct VggConvSpec { int index, cin, cout; };
constexpr VggConvSpec VGG_CONVS[9] = {{2, 3, 64},     {5, 64, 64},    {9, 64, 128},   {12, 128, 128}, {16, 128, 256},
                                      {19, 256, 256}, {22, 256, 256}, {25, 256, 256}, {29, 256, 512}};
inline int vgg_cinp(int cin) { return (cin + 3) / 4 * 4; }

struct VggTensor {
    size_t count;        // floats the caller hands over (the checkpoint's shape)
    size_t offset;       // floats into `weights`
    int conv;            // index into VGG_CONVS of a 3 x 3 weight (repacked at load), -1 otherwise
    bool loaded;
};

struct VggShape {
    int h[VGG_LEVELS], w[VGG_LEVELS];
    size_t in4, a, b, stat, total;          // float offsets of the workspace's parts; total in floats
};

bool vgg_shape(int H, int W, VggShape* s) {
    if (H < 9 || W < 9 || (int64_t)H * W > VGG_MAX_PIXELS) return false;         // 9 -> 5 -> 3 -> 2: every level's edge >= 2
    s->h[0] = H; s->w[0] = W;
    for (int l = 1; l < VGG_LEVELS; ++l) { s->h[l] = (s->h[l - 1] + 1) / 2; s->w[l] = (s->w[l - 1] + 1) / 2; }
    const size_t hw = (size_t)H * W;
    size_t big = hw * 64, stat = 0, at = 0;                                     // the widest maps are relu1_1 and relu1_2
    for (int l = 0; l < VGG_LEVELS; ++l) {
        big = std::max(big, (size_t)s->h[l] * s->w[l] * VGG_C[l]);
        stat = std::max(stat, vgg_mean_std_bytes((size_t)s->h[l] * s->w[l], VGG_C[l]) / sizeof(float));
    }
    auto take = [&](size_t n) { const size_t o = at; at += (n + 63) / 64 * 64; return o; };
    s->in4 = take(hw * 4); s->a = take(big); s->b = take(big); s->stat = take(stat);
    s->total = at;
    return true;
}

}  // namespace

struct vst_vgg {
    int device = -1;
    float* weights = nullptr;
    std::map<std::string, VggTensor> tensors;
    const float *w0 = nullptr, *b0 = nullptr, *cw[9] = {}, *cb[9] = {};
};

namespace {

#define VGG_TRY(expr)                    \
    do {                                 \
        const int rc__ = (expr);         \
        if (rc__ != VST_OK) return rc__; \
    } while (0)

// the whole chain in the caller's workspace: the four records, and relu4_1 where asked for
int vgg_features(vst_vgg* p, const void* frame, bool u8, int H, int W, double* records, float* relu4_1, void* ws_v,
                 size_t ws_bytes, hipStream_t st) {
    if (!frame || !vgg_f8(records) || ((uintptr_t)relu4_1 & 15)) return VST_E_ARG;
    if (!u8 && ((uintptr_t)frame & 3)) return VST_E_ARG;
    VggShape s;
    if (!vgg_shape(H, W, &s)) return VST_E_SHAPE;
    if (!vgg_f4(ws_v) || ws_bytes < s.total * sizeof(float)) return VST_E_WORKSPACE;
    if (!p) return VST_E_ARG;
    for (const auto& kv : p->tensors)
        if (!kv.second.loaded) return VST_E_ARG;
    int dev = -1;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return (int)e;
    if (dev != p->device) return VST_E_ARG;
    float* ws = static_cast<float*>(ws_v);
    float *in4 = ws + s.in4, *A = ws + s.a, *B = ws + s.b;
    double* stat = reinterpret_cast<double*>(ws + s.stat);
    double* rec[VGG_LEVELS] = {records, records + 128, records + 384, records + 896};
    float* last = relu4_1 ? relu4_1 : B;
    auto tap = [&](const float* map, int l) { return vgg_mean_std(map, (size_t)s.h[l] * s.w[l], VGG_C[l], 1e-5, rec[l], stat, st); };
    VGG_TRY(vgg_input(frame, u8, p->w0, p->b0, in4, H, W, st));
    VGG_TRY(vgg_conv(in4, p->cw[0], p->cb[0], A, s.h[0], s.w[0], 4, 64, st));             // relu1_1
    VGG_TRY(tap(A, 0));
    VGG_TRY(vgg_conv(A, p->cw[1], p->cb[1], B, s.h[0], s.w[0], 64, 64, st));
    VGG_TRY(vgg_maxpool(B, A, s.h[0], s.w[0], 64, st));
    VGG_TRY(vgg_conv(A, p->cw[2], p->cb[2], B, s.h[1], s.w[1], 64, 128, st));            // relu2_1
    VGG_TRY(tap(B, 1));
    VGG_TRY(vgg_conv(B, p->cw[3], p->cb[3], A, s.h[1], s.w[1], 128, 128, st));
    VGG_TRY(vgg_maxpool(A, B, s.h[1], s.w[1], 128, st));
    VGG_TRY(vgg_conv(B, p->cw[4], p->cb[4], A, s.h[2], s.w[2], 128, 256, st));           // relu3_1
    VGG_TRY(tap(A, 2));
    VGG_TRY(vgg_conv(A, p->cw[5], p->cb[5], B, s.h[2], s.w[2], 256, 256, st));
    VGG_TRY(vgg_conv(B, p->cw[6], p->cb[6], A, s.h[2], s.w[2], 256, 256, st));
    VGG_TRY(vgg_conv(A, p->cw[7], p->cb[7], B, s.h[2], s.w[2], 256, 256, st));
    VGG_TRY(vgg_maxpool(B, A, s.h[2], s.w[2], 256, st));
    VGG_TRY(vgg_conv(A, p->cw[8], p->cb[8], last, s.h[3], s.w[3], 256, 512, st));        // relu4_1
    VGG_TRY(tap(last, 3));
    return VST_OK;
}

}  // namespace

extern "C" {

// ---- kernel-level calls: the argument checks, then the launch helper the chain uses --------------------------------------
int vst_vgg_input_u8(const uint8_t* frame_hwc_u8, const float* w9, const float* b3, float* out, int H, int W, void* stream) {
    if (!frame_hwc_u8 || !w9 || !b3 || ((uintptr_t)w9 & 3) || ((uintptr_t)b3 & 3) || !vgg_f4(out)) return VST_E_ARG;
    if (H < 1 || W < 1 || (int64_t)H * W > VGG_MAX_PIXELS) return VST_E_SHAPE;
    return vgg_input(frame_hwc_u8, true, w9, b3, out, H, W, (hipStream_t)stream);
}

int vst_vgg_input_f32(const float* frame_planar, const float* w9, const float* b3, float* out, int H, int W, void* stream) {
    if (!frame_planar || ((uintptr_t)frame_planar & 3) || !w9 || !b3 || ((uintptr_t)w9 & 3) || ((uintptr_t)b3 & 3) || !vgg_f4(out))
        return VST_E_ARG;
    if (H < 1 || W < 1 || (int64_t)H * W > VGG_MAX_PIXELS) return VST_E_SHAPE;
    return vgg_input(frame_planar, false, w9, b3, out, H, W, (hipStream_t)stream);
}

int vst_vgg_conv3x3_relu(const float* in, const float* w, const float* bias, float* out, int H, int W, int Cin, int Cout,
                         void* stream) {
    if (!vgg_f4(in) || !vgg_f4(w) || !vgg_f4(bias) || !vgg_f4(out)) return VST_E_ARG;
    if (H < 2 || W < 2 || Cin < 4 || (Cin & 3) || Cout < 1 || (int64_t)H * W > VGG_MAX_PIXELS) return VST_E_SHAPE;
    const int64_t M = (int64_t)H * W;
    if (M * Cin > VGG_OP_MAX_FLOATS || M * Cout > VGG_OP_MAX_FLOATS || (int64_t)9 * Cin * Cout > VGG_OP_MAX_FLOATS ||
        (Cout + G_TILE - 1) / G_TILE > 65535)
        return VST_E_SHAPE;
    if (vgg_overlap(in, (size_t)M * Cin * sizeof(float), out, (size_t)M * Cout * sizeof(float))) return VST_E_ARG;
    return vgg_conv(in, w, bias, out, H, W, Cin, Cout, (hipStream_t)stream);
}

int vst_vgg_maxpool2(const float* in, float* out, int H, int W, int C, void* stream) {
    if (!vgg_f4(in) || !vgg_f4(out)) return VST_E_ARG;
    if (H < 1 || W < 1 || C < 4 || (C & 3) || (int64_t)H * W > VGG_MAX_PIXELS || (int64_t)H * W * C > VGG_OP_MAX_FLOATS)
        return VST_E_SHAPE;
    const size_t no = (size_t)((H + 1) / 2) * ((W + 1) / 2) * C * sizeof(float);
    if (vgg_overlap(in, (size_t)H * W * C * sizeof(float), out, no)) return VST_E_ARG;
    return vgg_maxpool(in, out, H, W, C, (hipStream_t)stream);
}

int vst_vgg_mean_std_workspace_bytes(int n, int C, size_t* bytes) {
    if (!bytes) return VST_E_ARG;
    if (n < 2 || C < 1 || (int64_t)n * C > VGG_OP_MAX_FLOATS) return VST_E_SHAPE;
    *bytes = vgg_mean_std_bytes((size_t)n, C);
    return VST_OK;
}

int vst_vgg_mean_std(const float* in, int n, int C, double eps, double* out, void* ws, size_t ws_bytes, void* stream) {
    if (!in || ((uintptr_t)in & 3) || !vgg_f8(out) || !(eps >= 0.0) || !(eps < 1e300)) return VST_E_ARG;
    if (n < 2 || C < 1 || (int64_t)n * C > VGG_OP_MAX_FLOATS) return VST_E_SHAPE;
    if (!vgg_f8(ws) || ws_bytes < vgg_mean_std_bytes((size_t)n, C)) return VST_E_WORKSPACE;
    return vgg_mean_std(in, (size_t)n, C, eps, out, static_cast<double*>(ws), (hipStream_t)stream);
}

int vst_vgg_mse_f64(const float* a, const float* b, size_t count, double* out, void* ws, void* stream) {
    if (!a || !b || (((uintptr_t)a | (uintptr_t)b) & 3) || !vgg_f8(out)) return VST_E_ARG;
    if (count < 1 || count > (size_t)VGG_OP_MAX_FLOATS) return VST_E_SHAPE;
    if (!vgg_f8(ws)) return VST_E_WORKSPACE;
    return vgg_mse(a, b, count, out, static_cast<double*>(ws), (hipStream_t)stream);
}

int vst_vgg_style_loss(const double* records_a, const double* records_b, double* out, void* stream) {
    if (!vgg_f8(records_a) || !vgg_f8(records_b) || !vgg_f8(out)) return VST_E_ARG;
    vgg_style_loss_kernel<<<1, 256, 0, (hipStream_t)stream>>>(records_a, records_b, out);
    VST_RETURN_IF_LAUNCH_FAILED();
    return VST_OK;
}

// ---- plan ------------------------------------------------------------------------------------------------------------------
int vst_vgg_create(vst_vgg** out) {
    if (!out) return VST_E_ARG;
    vst_vgg* p = new vst_vgg();
    hipError_t e = hipGetDevice(&p->device);
    if (e != hipSuccess) { delete p; return (int)e; }
    size_t at = 0;
    auto add = [&](const std::string& name, size_t count, size_t stored, int conv) {
        p->tensors[name] = VggTensor{count, at, conv, false};
        at += (stored + 63) / 64 * 64;
    };
    add("0.weight", 9, 9, -1);
    add("0.bias", 3, 3, -1);
    for (int i = 0; i < 9; ++i) {
        const VggConvSpec& c = VGG_CONVS[i];
        add(std::to_string(c.index) + ".weight", (size_t)c.cout * c.cin * 9, (size_t)c.cout * vgg_cinp(c.cin) * 9, i);
        add(std::to_string(c.index) + ".bias", c.cout, c.cout, -1);
    }
    e = hipMalloc(&p->weights, at * sizeof(float));
    if (e != hipSuccess) { delete p; return (int)e; }
    p->w0 = p->weights + p->tensors["0.weight"].offset;
    p->b0 = p->weights + p->tensors["0.bias"].offset;
    for (int i = 0; i < 9; ++i) {
        p->cw[i] = p->weights + p->tensors[std::to_string(VGG_CONVS[i].index) + ".weight"].offset;
        p->cb[i] = p->weights + p->tensors[std::to_string(VGG_CONVS[i].index) + ".bias"].offset;
    }
    *out = p;
    return VST_OK;
}

int vst_vgg_load_tensor(vst_vgg* p, const char* name, const float* data_host, size_t count) {
    if (!p || !name || !data_host) return VST_E_ARG;
    const auto it = p->tensors.find(name);
    if (it == p->tensors.end()) return VST_E_ARG;
    VggTensor& t = it->second;
    if (t.count != count) return VST_E_SHAPE;
    hipError_t e;
    if (t.conv >= 0) {          // [Cout][Cin][3][3] -> [Cout][ky][kx][Cin padded to 4 with zeros]
        const VggConvSpec& c = VGG_CONVS[t.conv];
        const int cp = vgg_cinp(c.cin);
        std::vector<float> packed((size_t)c.cout * 9 * cp, 0.f);
        for (int o = 0; o < c.cout; ++o)
            for (int i = 0; i < c.cin; ++i)
                for (int tp = 0; tp < 9; ++tp)
                    packed[((size_t)o * 9 + tp) * cp + i] = data_host[((size_t)o * c.cin + i) * 9 + tp];
        e = hipMemcpy(p->weights + t.offset, packed.data(), packed.size() * sizeof(float), hipMemcpyHostToDevice);
    } else {
        e = hipMemcpy(p->weights + t.offset, data_host, count * sizeof(float), hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) return (int)e;
    t.loaded = true;
    return VST_OK;
}

int vst_vgg_workspace_bytes(int H, int W, size_t* bytes) {
    if (!bytes) return VST_E_ARG;
    VggShape s;
    if (!vgg_shape(H, W, &s)) return VST_E_SHAPE;
    *bytes = s.total * sizeof(float);
    return VST_OK;
}

int vst_vgg_features_u8(vst_vgg* p, const uint8_t* frame_hwc_u8, int H, int W, double* records, float* relu4_1, void* ws,
                        size_t ws_bytes, void* stream) {
    return vgg_features(p, frame_hwc_u8, true, H, W, records, relu4_1, ws, ws_bytes, (hipStream_t)stream);
}

int vst_vgg_features_f32(vst_vgg* p, const float* frame_planar, int H, int W, double* records, float* relu4_1, void* ws,
                         size_t ws_bytes, void* stream) {
    return vgg_features(p, frame_planar, false, H, W, records, relu4_1, ws, ws_bytes, (hipStream_t)stream);
}

int vst_vgg_destroy(vst_vgg* p) {
    if (!p) return VST_E_ARG;
    if (p->weights) (void)hipFree(p->weights);
    delete p;
    return VST_OK;
}

}  // extern "C"
