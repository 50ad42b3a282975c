// SegFormer (MiT-B1..B5 backbone + MLP decode head) on gfx950: the segmenter of `image_transfer.py --auto_seg` and of the video
// loop, from a uint8 frame to a uint8 ADE20K label map without leaving the device ("On-device segmentation").
//
// Activations are token-major [tokens][C] fp32 (channels last) everywhere, so that every Linear and every conv with kernel =
// stride (or, after the patch gather, any conv) is one GEMM  out[M][N] = A[M][K] . W[N][K]^T + bias, and LayerNorm and the
// depthwise conv read contiguous channels.  The GEMM runs on bf16 MFMAs with split operands, like the stage-3 convs, but with a
// THREE-way split: x = hi + mid + lo (24 bits) and the six products hi.hi, hi.mid, mid.hi, mid.mid, hi.lo, lo.hi into fp32
// accumulators.  The two-way split (bf16x3) keeps 16 bits per operand; through this network that is 9-16 x the error of an fp32
// run, past the 8 x the label comparison allows ("On-device segmentation"); six products are fp32-class.
// Attention is a streaming softmax in fp32: the [N][Nk] scores never exist in memory.
#include "common.h"
#include <algorithm>
#include <map>
#include <mutex>
#include <string>
#include <vector>

namespace {

constexpr int SEG_CLASSES = 150;
constexpr int SEG_DIMS[4] = {64, 128, 320, 512};
constexpr int SEG_HEADS[4] = {1, 2, 5, 8};
constexpr int SEG_SR[4] = {8, 4, 2, 1};
constexpr int SEG_HEAD_DIM = 64;
static_assert(SEG_DIMS[0] == SEG_HEADS[0] * SEG_HEAD_DIM && SEG_DIMS[1] == SEG_HEADS[1] * SEG_HEAD_DIM &&
                  SEG_DIMS[2] == SEG_HEADS[2] * SEG_HEAD_DIM && SEG_DIMS[3] == SEG_HEADS[3] * SEG_HEAD_DIM,
              "seg_attention takes its heads from C / 64");
static_assert(SEG_DIMS[3] <= 512 && SEG_DIMS[0] <= SEG_DIMS[1] && SEG_DIMS[1] <= SEG_DIMS[2] && SEG_DIMS[2] <= SEG_DIMS[3],
              "seg_layernorm_kernel drops channels past 512");
constexpr int SEG_MAX_C = 512;          // widest token: seg_layernorm_kernel holds 8 channels per lane
constexpr int64_t SEG_MAX_PIXELS = (int64_t)1 << 24;      // whole-frame limit of the segmenter (4096 x 4096)
constexpr int64_t SEG_MAX_LABEL_PIXELS = VST_SEG_MAX_LABEL_PIXELS;      // limit of the label map a working frame is sampled to
constexpr int64_t SEG_MAX_LOGIT_CELLS = SEG_MAX_PIXELS / 16;

// ---------------------------------------------------------------------------------------------------------------- GEMM
// 64 x 64 output tile per workgroup, 4 waves; wave w owns rows 16w .. 16w+15 of the tile and all 64 columns (4 16 x 16 tiles, three accumulators each).
// MFMA operand A = activations (lane l: row l & 15, k = 8 (l >> 4) + j), operand B = weights (lane l: column l & 15, same k), so
// D has the output column in lane & 15: a store instruction writes four rows of 16 consecutive floats.
constexpr int G_TILE = 64;
constexpr int G_K = 32;
constexpr int G_LD = 40;        // bf16 per LDS row: 32 + 8 of padding (80 B, keeps ds_read_b128 aligned and spreads the banks)

__global__ __launch_bounds__(256) void seg_gemm_kernel(const float* __restrict__ A, const float* __restrict__ Wt,
                                                       const float* __restrict__ bias, const float* res, float* out, int M,
                                                       int N, int K) {
    __shared__ __attribute__((aligned(16))) __bf16 s_hi[2][G_TILE * G_LD];
    __shared__ __attribute__((aligned(16))) __bf16 s_md[2][G_TILE * G_LD];
    __shared__ __attribute__((aligned(16))) __bf16 s_lo[2][G_TILE * G_LD];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int m0 = blockIdx.x * G_TILE, n0 = blockIdx.y * G_TILE;
    const bool vec = (K & 3) == 0;
    // Three accumulators per output.  One fp32 sum fed all six products of every k-step is a chain of 6 K / 32 dependent MFMA
    // accumulations, each rounding the whole partial sum: 2.5 u of sum |a w| at K = 4096, 4.6 x an fp32 matmul's own error
    // (tests/test_gpu_segformer_ops.py).  hi.hi goes to big0 / big1 by the parity of the k-step (two chains of K / 64), the
    // five small products to `small`, where they round at their own magnitude (2^-8 of the sum); the epilogue adds the three.
    f32x4 big0[4], big1[4], small[4];
#pragma unroll
    for (int n = 0; n < 4; ++n) big0[n] = big1[n] = small[n] = f32x4{0.f, 0.f, 0.f, 0.f};

    auto k_step = [&](int k0, f32x4 (&big)[4]) {
        // stage 64 x 32 of A and of W: 2 x 512 groups of 4 consecutive k; rows past M / N and k past K are zeros
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int mat = i >> 1;
            const int g = tid + 256 * (i & 1);
            const int row = g >> 3, kq = (g & 7) * 4;
            const int r = (mat ? n0 : m0) + row;
            const int k = k0 + kq;
            float v[4] = {0.f, 0.f, 0.f, 0.f};
            if (r < (mat ? N : M)) {
                const float* p = (mat ? Wt : A) + (size_t)r * K + k;
                if (vec && k + 3 < K) {
                    const float4 t = *reinterpret_cast<const float4*>(p);
                    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (k + j < K) v[j] = p[j];
                }
            }
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
        const float b = bias ? bias[col] : 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = m0 + wave * 16 + (lane >> 4) * 4 + r;
            if (row >= M) continue;
            const size_t o = (size_t)row * N + col;
            float v = ((big0[n][r] + big1[n][r]) + small[n][r]) + b;
            if (res) v += res[o];          // res may alias out: every element is read and written by the same lane
            out[o] = v;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------- patch gathers
// First gather: the uint8 frame -> rows of patch_embed1's GEMM ([T1][7*7*3], K order (ky, kx, c)).  Does the work of the model's
// forward: replicate-pad right / bottom to (Hp, Wp), x / 255, ImageNet mean / std; the conv's own zero padding comes after that.
__global__ void seg_gather_rgb_kernel(const uint8_t* __restrict__ frame, int sy, int sx, int sc, int H, int W, int Hp, int Wp,
                                      int Ho, int Wo, float* __restrict__ col) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)Ho * Wo * 49) return;
    const int tap = (int)(idx % 49);
    const size_t row = idx / 49;
    const int oy = (int)(row / Wo), ox = (int)(row % Wo);
    const int iy = oy * 4 - 3 + tap / 7, ix = ox * 4 - 3 + tap % 7;
    float v[3] = {0.f, 0.f, 0.f};
    if (iy >= 0 && iy < Hp && ix >= 0 && ix < Wp) {
        const int cy = iy < H ? iy : H - 1, cx = ix < W ? ix : W - 1;
        const uint8_t* p = frame + (size_t)cy * sy + (size_t)cx * sx;
        const float mean[3] = {0.485f, 0.456f, 0.406f}, sd[3] = {0.229f, 0.224f, 0.225f};
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = ((float)p[(size_t)c * sc] / 255.f - mean[c]) / sd[c];
    }
    float* o = col + row * 147 + tap * 3;
    o[0] = v[0]; o[1] = v[1]; o[2] = v[2];
}

// token-major map [Hi*Wi][C] -> rows [Ho*Wo][k*k*C] of a k x k conv with the given stride and zero padding (C % 4 == 0)
__global__ void seg_im2col_kernel(const float* __restrict__ in, int Hi, int Wi, int C, int k, int stride, int pad, int Ho,
                                  int Wo, float* __restrict__ col) {
    const int c4n = C >> 2;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t per_row = (size_t)k * k * c4n;
    if (idx >= (size_t)Ho * Wo * per_row) return;
    const size_t row = idx / per_row;
    const int rem = (int)(idx % per_row);
    const int tap = rem / c4n, c4 = rem % c4n;
    const int oy = (int)(row / Wo), ox = (int)(row % Wo);
    const int iy = oy * stride - pad + tap / k, ix = ox * stride - pad + tap % k;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (iy >= 0 && iy < Hi && ix >= 0 && ix < Wi)
        v = *reinterpret_cast<const float4*>(in + ((size_t)iy * Wi + ix) * C + c4 * 4);
    *reinterpret_cast<float4*>(col + row * ((size_t)k * k * C) + (size_t)tap * C + c4 * 4) = v;
}

// --------------------------------------------------------------------------------------------------------------- LayerNorm
// one wave per token, C <= 512: the token sits in registers, mean and variance in two passes over them (out may alias x)
__global__ __launch_bounds__(256) void seg_layernorm_kernel(const float* x, const float* __restrict__ g,
                                                            const float* __restrict__ b, float* out, int T, int C, float eps) {
    const int lane = threadIdx.x & 63;
    const size_t t = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= (size_t)T) return;
    float v[8], s = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int c = lane + 64 * i;
        v[i] = c < C ? x[t * C + c] : 0.f;
        s += v[i];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    const float mean = s / (float)C;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float d = (lane + 64 * i) < C ? v[i] - mean : 0.f;
        q += d * d;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o, 64);
    const float rstd = 1.f / sqrtf(q / (float)C + eps);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int c = lane + 64 * i;
        if (c < C) out[t * C + c] = (v[i] - mean) * rstd * g[c] + b[c];
    }
}

// --------------------------------------------------------------------------------------------------------------- attention
// head_dim 64.  A lane owns one query row of one head: q (scaled), the running max / sum and the 64 output sums live in its
// registers.  The workgroup (128 rows of one head) walks K / V in chunks of 16 keys staged in LDS; every lane reads the same
// key, so the LDS reads are broadcasts.  kv = [Nk][2C]: K of head h at column 64 h, V at C + 64 h.
constexpr int AT_ROWS = 128;
constexpr int AT_KEYS = 16;

__global__ __launch_bounds__(AT_ROWS) void seg_attention_kernel(const float* __restrict__ q, const float* __restrict__ kv,
                                                                float* __restrict__ out, int N, int Nk, int C, float scale) {
    __shared__ __attribute__((aligned(16))) float s_k[AT_KEYS][SEG_HEAD_DIM];
    __shared__ __attribute__((aligned(16))) float s_v[AT_KEYS][SEG_HEAD_DIM];
    const int tid = threadIdx.x, h = blockIdx.y;
    const size_t row = (size_t)blockIdx.x * AT_ROWS + tid;
    const bool live = row < (size_t)N;
    const size_t rr = live ? row : (size_t)N - 1;
    float qv[SEG_HEAD_DIM], acc[SEG_HEAD_DIM];
#pragma unroll
    for (int d = 0; d < SEG_HEAD_DIM; d += 4) {
        const float4 t = *reinterpret_cast<const float4*>(q + rr * C + h * SEG_HEAD_DIM + d);
        qv[d] = t.x * scale; qv[d + 1] = t.y * scale; qv[d + 2] = t.z * scale; qv[d + 3] = t.w * scale;
        acc[d] = acc[d + 1] = acc[d + 2] = acc[d + 3] = 0.f;
    }
    float m = -INFINITY, l = 0.f;
    for (int k0 = 0; k0 < Nk; k0 += AT_KEYS) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int g = tid + AT_ROWS * i;           // 16 keys x (16 float4 of K + 16 float4 of V)
            const int key = g >> 5, part = g & 31;
            const int kk = k0 + key;
            float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
            const int colv = (part < 16 ? 0 : C) + h * SEG_HEAD_DIM + (part & 15) * 4;
            if (kk < Nk) t = *reinterpret_cast<const float4*>(kv + (size_t)kk * 2 * C + colv);
            float* dst = part < 16 ? &s_k[key][(part & 15) * 4] : &s_v[key][(part & 15) * 4];
            *reinterpret_cast<float4*>(dst) = t;
        }
        __syncthreads();
        const int nk = Nk - k0 < AT_KEYS ? Nk - k0 : AT_KEYS;
        float s[AT_KEYS], cm = -INFINITY;
#pragma unroll
        for (int j = 0; j < AT_KEYS; ++j) {
            float dot = 0.f;
#pragma unroll
            for (int d = 0; d < SEG_HEAD_DIM; d += 4) {
                const float4 kq = *reinterpret_cast<const float4*>(&s_k[j][d]);
                dot = fmaf(qv[d], kq.x, dot); dot = fmaf(qv[d + 1], kq.y, dot);
                dot = fmaf(qv[d + 2], kq.z, dot); dot = fmaf(qv[d + 3], kq.w, dot);
            }
            s[j] = j < nk ? dot : -INFINITY;
            cm = fmaxf(cm, s[j]);
        }
        const float mn = fmaxf(m, cm);              // finite: a chunk holds at least one key
        const float corr = expf(m - mn);            // 0 on the first chunk
        l *= corr;
#pragma unroll
        for (int d = 0; d < SEG_HEAD_DIM; ++d) acc[d] *= corr;
#pragma unroll
        for (int j = 0; j < AT_KEYS; ++j) {
            const float p = expf(s[j] - mn);        // 0 for the keys past Nk
            l += p;
#pragma unroll
            for (int d = 0; d < SEG_HEAD_DIM; d += 4) {
                const float4 vv = *reinterpret_cast<const float4*>(&s_v[j][d]);
                acc[d] = fmaf(p, vv.x, acc[d]); acc[d + 1] = fmaf(p, vv.y, acc[d + 1]);
                acc[d + 2] = fmaf(p, vv.z, acc[d + 2]); acc[d + 3] = fmaf(p, vv.w, acc[d + 3]);
            }
        }
        m = mn;
    }
    if (!live) return;
    const float inv = 1.f / l;
#pragma unroll
    for (int d = 0; d < SEG_HEAD_DIM; d += 4)
        *reinterpret_cast<float4*>(out + row * C + h * SEG_HEAD_DIM + d) =
            make_float4(acc[d] * inv, acc[d + 1] * inv, acc[d + 2] * inv, acc[d + 3] * inv);
}

// ------------------------------------------------------------------------------------- depthwise 3x3 + bias + exact GELU
// Mlp.dwconv + Mlp.act on the token-major [H*W][C] map, zero-padded borders; w = [9][C] (tap-major), C % 4 == 0
__device__ __forceinline__ float gelu_erf(float x) { return 0.5f * x * (1.f + erff(x * 0.70710678118654752440f)); }

__global__ void seg_dwconv_gelu_kernel(const float* __restrict__ in, const float* __restrict__ w, const float* __restrict__ b,
                                       float* __restrict__ out, int H, int W, int C) {
    const int c4n = C >> 2;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)H * W * c4n) return;
    const int c = (int)(idx % c4n) * 4;
    const size_t pix = idx / c4n;
    const int y = (int)(pix / W), x = (int)(pix % W);
    float4 a = *reinterpret_cast<const float4*>(b + c);
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const int iy = y + t / 3 - 1, ix = x + t % 3 - 1;
        if (iy < 0 || iy >= H || ix < 0 || ix >= W) continue;
        const float4 v = *reinterpret_cast<const float4*>(in + ((size_t)iy * W + ix) * C + c);
        const float4 k = *reinterpret_cast<const float4*>(w + (size_t)t * C + c);
        a.x = fmaf(v.x, k.x, a.x); a.y = fmaf(v.y, k.y, a.y); a.z = fmaf(v.z, k.z, a.z); a.w = fmaf(v.w, k.w, a.w);
    }
    *reinterpret_cast<float4*>(out + pix * C + c) = make_float4(gelu_erf(a.x), gelu_erf(a.y), gelu_erf(a.z), gelu_erf(a.w));
}

// ------------------------------------------------------------------------------------------------------------ decode head
// F.interpolate(mode="bilinear", align_corners=False) source taps of output index `dst` for in -> out
struct Taps { int i0, i1; float l; };
__device__ __forceinline__ Taps bilinear_taps(int dst, int in, int out) {
    float s = fmaf((float)in / (float)out, (float)dst + 0.5f, -0.5f);      // (one rounding, at every call site)
    s = s < 0.f ? 0.f : s;
    Taps t;
    t.i0 = (int)s;
    t.i0 = t.i0 > in - 1 ? in - 1 : t.i0;
    t.i1 = t.i0 < in - 1 ? t.i0 + 1 : t.i0;
    t.l = s - (float)t.i0;
    return t;
}

struct HeadMaps { const float* y[4]; int h[4], w[4]; };

// out = ReLU(y[0] + upsample(y[1]) + upsample(y[2]) + upsample(y[3])) on y[0]'s grid; out may be y[0] (a thread reads its own
// float4 of y[0] before it stores it); E % 4 == 0
__global__ void seg_head_sum_kernel(HeadMaps mp, float* out, int E) {
    const int e4n = E >> 2;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)mp.h[0] * mp.w[0] * e4n) return;
    const int c = (int)(idx % e4n) * 4;
    const size_t pix = idx / e4n;
    const int y = (int)(pix / mp.w[0]), x = (int)(pix % mp.w[0]);
    float4 a = *reinterpret_cast<const float4*>(mp.y[0] + pix * E + c);
#pragma unroll
    for (int s = 1; s < 4; ++s) {
        const Taps ty = bilinear_taps(y, mp.h[s], mp.h[0]), tx = bilinear_taps(x, mp.w[s], mp.w[0]);
        const float* base = mp.y[s] + c;
        const float4 v00 = *reinterpret_cast<const float4*>(base + ((size_t)ty.i0 * mp.w[s] + tx.i0) * E);
        const float4 v01 = *reinterpret_cast<const float4*>(base + ((size_t)ty.i0 * mp.w[s] + tx.i1) * E);
        const float4 v10 = *reinterpret_cast<const float4*>(base + ((size_t)ty.i1 * mp.w[s] + tx.i0) * E);
        const float4 v11 = *reinterpret_cast<const float4*>(base + ((size_t)ty.i1 * mp.w[s] + tx.i1) * E);
        const float w00 = (1.f - ty.l) * (1.f - tx.l), w01 = (1.f - ty.l) * tx.l, w10 = ty.l * (1.f - tx.l), w11 = ty.l * tx.l;
        a.x += w00 * v00.x + w01 * v01.x + w10 * v10.x + w11 * v11.x;
        a.y += w00 * v00.y + w01 * v01.y + w10 * v10.y + w11 * v11.y;
        a.z += w00 * v00.z + w01 * v01.z + w10 * v10.z + w11 * v11.z;
        a.w += w00 * v00.w + w01 * v01.w + w10 * v10.w + w11 * v11.w;
    }
    *reinterpret_cast<float4*>(out + pix * E + c) = make_float4(fmaxf(a.x, 0.f), fmaxf(a.y, 0.f), fmaxf(a.z, 0.f), fmaxf(a.w, 0.f));
}

// The four-tap sum of the two samplers below: every product and every sum rounded, in this order.  Contraction into FMAs is
// off, so that both kernels compute the same bits whatever surrounds the expression.
__device__ __forceinline__ float seg_blend(float w00, float v00, float w01, float v01, float w10, float v10, float w11, float v11) {
#pragma clang fp contract(off)
    return w00 * v00 + w01 * v01 + w10 * v10 + w11 * v11;
}

// quarter-resolution logits [Hq*Wq][150] -> labels uint8 [H][W]: bilinear sample as F.interpolate(size=(H, W)) does, argmax over
// the classes (lowest index on ties; softmax is monotone and skipped).  16 lanes per pixel, each takes every 16th class.
__global__ __launch_bounds__(256) void seg_argmax_kernel(const float* __restrict__ lg, int Hq, int Wq, int H, int W,
                                                         uint8_t* __restrict__ labels) {
    const int sub = threadIdx.x & 15;
    const size_t n = (size_t)H * W;
    size_t pix = ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 16 + (threadIdx.x >> 4);      // (seg_grid: y > 0 past 2^24 pixels)
    const bool live = pix < n;
    if (!live) pix = n - 1;
    const int y = (int)(pix / W), x = (int)(pix % W);
    const Taps ty = bilinear_taps(y, Hq, H), tx = bilinear_taps(x, Wq, W);
    const float* p00 = lg + ((size_t)ty.i0 * Wq + tx.i0) * SEG_CLASSES;
    const float* p01 = lg + ((size_t)ty.i0 * Wq + tx.i1) * SEG_CLASSES;
    const float* p10 = lg + ((size_t)ty.i1 * Wq + tx.i0) * SEG_CLASSES;
    const float* p11 = lg + ((size_t)ty.i1 * Wq + tx.i1) * SEG_CLASSES;
    const float w00 = (1.f - ty.l) * (1.f - tx.l), w01 = (1.f - ty.l) * tx.l, w10 = ty.l * (1.f - tx.l), w11 = ty.l * tx.l;
    float best = -INFINITY;
    int bi = SEG_CLASSES;
    for (int c = sub; c < SEG_CLASSES; c += 16) {
        const float v = seg_blend(w00, p00[c], w01, p01[c], w10, p10[c], w11, p11[c]);
        if (v > best) { best = v; bi = c; }
    }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
    }
    if (live && sub == 0) labels[pix] = (uint8_t)(bi < SEG_CLASSES ? bi : 0);
}

// The same map from the same logits for LARGE upsampling factors (a frame segmented at a working resolution, DESIGN.md
// "Working resolution"): above, every pixel fetches its four cells (4 x 150 floats) from global memory, and at 15 x a cell is
// fetched by ~900 pixels.  Here a workgroup owns UP_TW x UP_TH output pixels, stages the cells [cy0, cy1] x [cx0, cx1] its
// taps touch into LDS once (taps are monotone in the pixel index, so the tile's first and last pixel give the range), and every
// pixel then reads LDS.  One lane per pixel, all 150 classes in ascending order with a strict `>`: the lowest index of the
// maximum, which is what the 16-lane scan and its reduction above return.  Taps, weights and the four-term sum (seg_blend) are
// those of the kernel above, so the labels are the same bytes.
// LDS layout: cell (cy, cx) at ((cy - cy0) * ncx + (cx - cx0)) * 150 floats, unpadded.  A wave reads one class pair (8 B) of
// the cells of 64 consecutive pixels of ONE row with ds_read_b64: bank (a / 4) % 64 per 32-lane half, cell stride 150 dwords
// = 22 mod 64, so consecutive cells start on banks 0, 22, 44, 2, 24, ... - even, distinct for 32 cells in a row; equal
// addresses broadcast.  A half-wave touches at most 32 / scale + 2 cells, so the reads are conflict-free without padding.
// The host bounds the cell count (seg_up_cells) and passes the LDS size; scales under 4 per axis do not fit and are refused.
constexpr int UP_TW = 64, UP_TH = 16;
constexpr int UP_MAX_CELLS = 108;          // (63 / 4 + 3) * (15 / 4 + 3): 64,800 B, the scale-4 tile

// one pixel's classes in ascending order from its four cells (LDS or global memory after inlining)
__device__ __forceinline__ uint8_t seg_up_scan(const float* p00, const float* p01, const float* p10, const float* p11, float w00,
                                               float w01, float w10, float w11) {
    float best = -INFINITY;
    int bi = SEG_CLASSES;
    for (int c = 0; c < SEG_CLASSES; c += 2) {
        const float2 a00 = *reinterpret_cast<const float2*>(p00 + c), a01 = *reinterpret_cast<const float2*>(p01 + c);
        const float2 a10 = *reinterpret_cast<const float2*>(p10 + c), a11 = *reinterpret_cast<const float2*>(p11 + c);
        const float v0 = seg_blend(w00, a00.x, w01, a01.x, w10, a10.x, w11, a11.x);
        const float v1 = seg_blend(w00, a00.y, w01, a01.y, w10, a10.y, w11, a11.y);
        if (v0 > best) { best = v0; bi = c; }
        if (v1 > best) { best = v1; bi = c + 1; }
    }
    return (uint8_t)(bi < SEG_CLASSES ? bi : 0);
}

// cap_y x cap_x: the cells the launch's LDS holds (seg_up_cells).  The bound is exact in real arithmetic; should the float
// coordinate's rounding ever make a tile touch one cell more, the pixels that need it read global memory like the kernel above.
__global__ __launch_bounds__(256) void seg_argmax_up_kernel(const float* __restrict__ lg, int Hq, int Wq, int H, int W,
                                                            unsigned tiles_x, int cap_y, int cap_x, uint8_t* __restrict__ labels) {
    extern __shared__ float up_cells[];
    const size_t tile = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    const int x0 = (int)(tile % tiles_x) * UP_TW, y0 = (int)(tile / tiles_x) * UP_TH;
    if (y0 >= H) return;                            // (the last grid row of seg_grid may be ragged; uniform per workgroup)
    const int x1 = min(x0 + UP_TW, W) - 1, y1 = min(y0 + UP_TH, H) - 1;
    const int cy0 = bilinear_taps(y0, Hq, H).i0, cx0 = bilinear_taps(x0, Wq, W).i0;
    const int ncy = min(bilinear_taps(y1, Hq, H).i1 - cy0 + 1, cap_y), ncx = min(bilinear_taps(x1, Wq, W).i1 - cx0 + 1, cap_x);
    const int row2 = ncx * (SEG_CLASSES / 2);
    for (int r = 0; r < ncy; ++r) {                 // a row of cells is contiguous in memory
        const float2* src = reinterpret_cast<const float2*>(lg + ((size_t)(cy0 + r) * Wq + cx0) * SEG_CLASSES);
        float2* dst = reinterpret_cast<float2*>(up_cells) + r * row2;
        for (int i = threadIdx.x; i < row2; i += 256) dst[i] = src[i];
    }
    __syncthreads();
    const int x = x0 + (threadIdx.x & 63);
    if (x > x1) return;
    const Taps tx = bilinear_taps(x, Wq, W);
    for (int y = y0 + (threadIdx.x >> 6); y <= y1; y += 4) {
        const Taps ty = bilinear_taps(y, Hq, H);
        const float w00 = (1.f - ty.l) * (1.f - tx.l), w01 = (1.f - ty.l) * tx.l, w10 = ty.l * (1.f - tx.l), w11 = ty.l * tx.l;
        uint8_t label;
        if (ty.i0 >= cy0 && tx.i0 >= cx0 && ty.i1 - cy0 < ncy && tx.i1 - cx0 < ncx) {
            const float* r0 = up_cells + (ty.i0 - cy0) * ncx * SEG_CLASSES;
            const float* r1 = up_cells + (ty.i1 - cy0) * ncx * SEG_CLASSES;
            label = seg_up_scan(r0 + (tx.i0 - cx0) * SEG_CLASSES, r0 + (tx.i1 - cx0) * SEG_CLASSES, r1 + (tx.i0 - cx0) * SEG_CLASSES,
                                r1 + (tx.i1 - cx0) * SEG_CLASSES, w00, w01, w10, w11);
        } else {
            label = seg_up_scan(lg + ((size_t)ty.i0 * Wq + tx.i0) * SEG_CLASSES, lg + ((size_t)ty.i0 * Wq + tx.i1) * SEG_CLASSES,
                                lg + ((size_t)ty.i1 * Wq + tx.i0) * SEG_CLASSES, lg + ((size_t)ty.i1 * Wq + tx.i1) * SEG_CLASSES,
                                w00, w01, w10, w11);
        }
        labels[(size_t)y * W + x] = label;
    }
}

// ---------------------------------------------------------------------------------------------------------------- temporal mix
// out[i] = w[0] * x0[i] + w[1] * x1[i] + ... over the logits of up to SEG_MIX_MAX frames (vst_seg_mix_logits; DESIGN.md,
// "Temporal window").  Pointers and weights are kernel arguments: no table in device memory.  Every product and every sum is
// rounded to fp32, in increasing age, so a caller can restate the chain exactly; 1.f * x is x, so one frame of weight 1 is a copy.
// Elementwise and memory-bound: V = float4 where every pointer is 16-byte aligned, else float2 (8 bytes is what the entry
// guarantees); the last count % (sizeof(V) / 4) floats are done one by one.
constexpr int SEG_MIX_MAX = VST_SEG_MIX_MAX;
constexpr unsigned SEG_MIX_MAX_BLOCKS = 256 * 8;       // 256 CUs x 8 workgroups of 256 threads: a grid-stride loop beyond that
struct SegMixArgs {
    const float* x[SEG_MIX_MAX];
    float w[SEG_MIX_MAX];
};

template <int N>
__device__ __forceinline__ float seg_mix_chain(const float (&v)[N], const float (&w)[SEG_MIX_MAX]) {
#pragma clang fp contract(off)
    float acc = w[0] * v[0];
#pragma unroll
    for (int k = 1; k < N; ++k) acc = acc + w[k] * v[k];
    return acc;
}

template <int N, typename V>
__global__ __launch_bounds__(256) void seg_mix_kernel(SegMixArgs a, size_t count, float* __restrict__ out) {
    constexpr int L = sizeof(V) / sizeof(float);
    const size_t nvec = count / L;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += stride) {
        V in[N];
#pragma unroll
        for (int k = 0; k < N; ++k) in[k] = reinterpret_cast<const V*>(a.x[k])[i];
        V r;
#pragma unroll
        for (int j = 0; j < L; ++j) {
            float v[N];
#pragma unroll
            for (int k = 0; k < N; ++k) v[k] = reinterpret_cast<const float*>(&in[k])[j];
            reinterpret_cast<float*>(&r)[j] = seg_mix_chain<N>(v, a.w);
        }
        reinterpret_cast<V*>(out)[i] = r;
    }
    if (blockIdx.x == 0) {
        for (size_t i = nvec * L + threadIdx.x; i < count; i += blockDim.x) {
            float v[N];
#pragma unroll
            for (int k = 0; k < N; ++k) v[k] = a.x[k][i];
            out[i] = seg_mix_chain<N>(v, a.w);
        }
    }
}

template <int N>
void seg_mix_launch(const SegMixArgs& a, size_t count, float* out, bool wide, hipStream_t st) {
    const size_t nvec = count / (wide ? 4 : 2);
    const unsigned blocks = (unsigned)std::min<size_t>(std::max<size_t>((nvec + 255) / 256, 1), SEG_MIX_MAX_BLOCKS);
    if (wide)
        seg_mix_kernel<N, float4><<<blocks, 256, 0, st>>>(a, count, out);
    else
        seg_mix_kernel<N, float2><<<blocks, 256, 0, st>>>(a, count, out);
}

// ---------------------------------------------------------------------------------------------------------------- the plan
struct SegBlock {
    float *n1w, *n1b, *qw, *qb, *kvw, *kvb, *srw, *srb, *snw, *snb, *pw, *pb, *n2w, *n2b, *f1w, *f1b, *dww, *dwb, *f2w, *f2b;
};
struct SegStage {
    float *pew, *peb, *penw, *penb, *nw, *nb;
    std::vector<SegBlock> blocks;
};
struct SegTensor {
    std::string name;
    size_t count, offset;
    float** slot;
    bool loaded;
};
struct SegArena {
    float* base = nullptr;
    size_t floats = 0;
};
struct SegShape {
    int H, W, Hp, Wp, h[4], w[4], hk[4], wk[4];
    size_t T[4], Tk[4];
    size_t x, xn, q, col, sr, kv, h1, h2, xs[4], y[4], lg, total;     // float offsets into the arena
};

}  // namespace

struct vst_seg {
    int device, depths[4], E;
    SegStage st[4];
    float *fold[4], *foldb, *predw, *predb;
    float* weights = nullptr;
    std::vector<SegTensor> tensors;
    std::map<std::string, int> index;
    std::mutex mu;
    std::map<hipStream_t, SegArena> arenas;       // one workspace per stream (the plan belongs to one device)
};

namespace {

void seg_register(vst_seg* p, const std::string& name, size_t count, float** slot) {
    p->index[name] = (int)p->tensors.size();
    p->tensors.push_back(SegTensor{name, count, 0, slot, false});
}

bool seg_shape(int H, int W, SegShape* s) {
    if (H < 32 || W < 32 || (int64_t)H * W > SEG_MAX_PIXELS) return false;
    s->H = H; s->W = W;
    s->Hp = (H + 3) / 4 * 4; s->Wp = (W + 3) / 4 * 4;
    s->h[0] = s->Hp / 4; s->w[0] = s->Wp / 4;
    for (int i = 1; i < 4; ++i) { s->h[i] = (s->h[i - 1] - 1) / 2 + 1; s->w[i] = (s->w[i - 1] - 1) / 2 + 1; }
    for (int i = 0; i < 4; ++i) {
        s->hk[i] = s->h[i] / SEG_SR[i]; s->wk[i] = s->w[i] / SEG_SR[i];
        if (s->hk[i] < 1 || s->wk[i] < 1) return false;
        s->T[i] = (size_t)s->h[i] * s->w[i];
        s->Tk[i] = (size_t)s->hk[i] * s->wk[i];
    }
    return true;
}

void seg_carve(SegShape* s, int E) {
    size_t tc = 0, col = s->T[0] * 147, sr = 0, kv = 0;
    for (int i = 0; i < 4; ++i) {
        const size_t C = SEG_DIMS[i];
        tc = std::max(tc, s->T[i] * C);
        if (i > 0) col = std::max(col, s->T[i] * 9 * SEG_DIMS[i - 1]);
        col = std::max(col, s->Tk[i] * SEG_SR[i] * SEG_SR[i] * C);
        sr = std::max(sr, s->Tk[i] * C);
        kv = std::max(kv, s->Tk[i] * 2 * C);
    }
    size_t at = 0;
    auto take = [&](size_t n) { const size_t o = at; at += (n + 63) / 64 * 64; return o; };
    s->x = take(tc); s->xn = take(tc); s->q = take(tc); s->col = take(col); s->sr = take(sr); s->kv = take(kv);
    s->h1 = take(tc * 4); s->h2 = take(tc * 4);
    for (int i = 0; i < 4; ++i) s->xs[i] = take(s->T[i] * SEG_DIMS[i]);
    for (int i = 0; i < 4; ++i) s->y[i] = take(s->T[i] * E);
    s->lg = take(s->T[0] * SEG_CLASSES);
    s->total = at;
}

// the stream's workspace, grown when a larger frame arrives (growing waits for the stream's earlier work: first use only)
int seg_arena(vst_seg* p, hipStream_t st, size_t floats, float** base) {
    std::lock_guard<std::mutex> lock(p->mu);
    SegArena& a = p->arenas[st];
    if (a.floats < floats) {
        if (a.base) {
            hipError_t e = hipStreamSynchronize(st);
            if (e != hipSuccess) return (int)e;
            (void)hipFree(a.base);
            a.base = nullptr; a.floats = 0;
        }
        hipError_t e = hipMalloc(&a.base, floats * sizeof(float));
        if (e != hipSuccess) return (int)e;
        a.floats = floats;
    }
    *base = a.base;
    return VST_OK;
}

inline unsigned blocks_for(size_t n, int per) { return (unsigned)((n + per - 1) / per); }

int seg_gemm(const float* A, const float* W, const float* bias, const float* res, float* out, size_t M, int N, int K,
             hipStream_t st) {
    dim3 grid(blocks_for(M, G_TILE), blocks_for((size_t)N, G_TILE));
    seg_gemm_kernel<<<grid, 256, 0, st>>>(A, W, bias, res, out, (int)M, N, K);
    VST_RETURN_IF_LAUNCH_FAILED();
    return VST_OK;
}
int seg_ln(const float* x, const float* g, const float* b, float* out, size_t T, int C, float eps, hipStream_t st) {
    seg_layernorm_kernel<<<blocks_for(T, 4), 256, 0, st>>>(x, g, b, out, (int)T, C, eps);
    VST_RETURN_IF_LAUNCH_FAILED();
    return VST_OK;
}
int seg_im2col(const float* in, int Hi, int Wi, int C, int k, int stride, int pad, int Ho, int Wo, float* col, hipStream_t st) {
    const size_t n = (size_t)Ho * Wo * k * k * (C / 4);
    seg_im2col_kernel<<<blocks_for(n, 256), 256, 0, st>>>(in, Hi, Wi, C, k, stride, pad, Ho, Wo, col);
    VST_RETURN_IF_LAUNCH_FAILED();
    return VST_OK;
}
int seg_gather_rgb(const uint8_t* frame, int chw, const SegShape& s, float* col, hipStream_t st) {
    const int H = s.H, W = s.W;
    const int sy = chw ? W : W * 3, sx = chw ? 1 : 3, sc = chw ? H * W : 1;
    seg_gather_rgb_kernel<<<blocks_for(s.T[0] * 49, 256), 256, 0, st>>>(frame, sy, sx, sc, H, W, s.Hp, s.Wp, s.h[0], s.w[0], col);
    VST_RETURN_IF_LAUNCH_FAILED();
    return VST_OK;
}
// heads = C / 64; a workgroup per AT_ROWS query rows and head
int seg_attention(const float* q, const float* kv, float* out, size_t N, size_t Nk, int C, float scale, hipStream_t st) {
    seg_attention_kernel<<<dim3(blocks_for(N, AT_ROWS), C / SEG_HEAD_DIM), AT_ROWS, 0, st>>>(q, kv, out, (int)N, (int)Nk, C, scale);
    VST_RETURN_IF_LAUNCH_FAILED();
    return VST_OK;
}
// C = the channels of the map (the Mlp's hidden width, 4 x the stage's), one thread per float4
int seg_dwconv_gelu(const float* in, const float* w, const float* b, float* out, int H, int W, int C, hipStream_t st) {
    seg_dwconv_gelu_kernel<<<blocks_for((size_t)H * W * (C / 4), 256), 256, 0, st>>>(in, w, b, out, H, W, C);
    VST_RETURN_IF_LAUNCH_FAILED();
    return VST_OK;
}
int seg_head_sum(const HeadMaps& mp, float* out, int E, hipStream_t st) {
    seg_head_sum_kernel<<<blocks_for((size_t)mp.h[0] * mp.w[0] * (E / 4), 256), 256, 0, st>>>(mp, out, E);
    VST_RETURN_IF_LAUNCH_FAILED();
    return VST_OK;
}

// An upper bound of the cells a UP_TW x UP_TH tile stages: the source coordinate moves by (n - 1) * in / out over n pixels, the
// first tap is its floor and the second tap one more; one further cell covers the rounding of the float coordinate.
// `blocks` workgroups as a grid of at most 2^20 per row: a 1-D grid of more than 2^24 workgroups of 256 threads passes 2^32
// threads, which the runtime does not launch in full.  The kernels index with blockIdx.y * gridDim.x + blockIdx.x and drop the
// ragged end of the last row; up to 2^20 workgroups (every frame of at most 2^24 pixels) the grid is the 1-D grid it was.
dim3 seg_grid(size_t blocks) {
    const size_t gx = std::min<size_t>(blocks, (size_t)1 << 20);
    return dim3((unsigned)gx, (unsigned)((blocks + gx - 1) / gx));
}

void seg_up_cells(int Hq, int Wq, int H, int W, int* ny, int* nx) {
    *ny = (int)std::min<int64_t>(Hq, (int64_t)(UP_TH - 1) * Hq / H + 3);
    *nx = (int)std::min<int64_t>(Wq, (int64_t)(UP_TW - 1) * Wq / W + 3);
}

// A run takes the tiled sampler from this upsampling factor on, on both axes (H >= T * Hq and W >= T * Wq); 0 = never.  The
// threshold is to be the smallest measured factor from which the tiled sampler is faster (tools/bench_segment.py --argmax_ab).
// It has not been measured yet ("Working resolution"), so the tiled sampler is selectable (kernel = 1) but not dispatched.
constexpr int SEG_UP_MIN_SCALE = 0;

// kernel: 0 = per pixel, 1 = tiled, -1 = by scale
int seg_labels(const float* lg, int Hq, int Wq, int H, int W, int kernel, uint8_t* labels, hipStream_t st) {
    if (kernel < -1 || kernel > 1) return VST_E_ARG;
    int ny, nx;
    seg_up_cells(Hq, Wq, H, W, &ny, &nx);
    const int cells = ny * nx <= UP_MAX_CELLS ? ny * nx : UP_MAX_CELLS + 1;
    if (kernel < 0)
        kernel = SEG_UP_MIN_SCALE > 0 && cells <= UP_MAX_CELLS && (int64_t)H >= (int64_t)SEG_UP_MIN_SCALE * Hq &&
                 (int64_t)W >= (int64_t)SEG_UP_MIN_SCALE * Wq;
    if (kernel == 1) {
        if (cells > UP_MAX_CELLS) return VST_E_SHAPE;
        const unsigned tiles_x = blocks_for((size_t)W, UP_TW);
        seg_argmax_up_kernel<<<seg_grid((size_t)tiles_x * blocks_for((size_t)H, UP_TH)), 256, (size_t)cells * SEG_CLASSES * sizeof(float), st>>>(
            lg, Hq, Wq, H, W, tiles_x, ny, nx, labels);
    } else {
        seg_argmax_kernel<<<seg_grid(((size_t)H * W + 15) / 16), 256, 0, st>>>(lg, Hq, Wq, H, W, labels);
    }
    VST_RETURN_IF_LAUNCH_FAILED();
    return VST_OK;
}

#define SEG_TRY(expr)                  \
    do {                               \
        const int rc__ = (expr);       \
        if (rc__ != VST_OK) return rc__; \
    } while (0)

// the whole network up to the quarter-resolution logits, in the arena `ws` carved by `s`
int seg_forward(vst_seg* p, const uint8_t* frame, int chw, const SegShape& s, float* ws, hipStream_t st) {
    float *x = ws + s.x, *xn = ws + s.xn, *q = ws + s.q, *col = ws + s.col, *srb = ws + s.sr, *kv = ws + s.kv;
    float *h1 = ws + s.h1, *h2 = ws + s.h2;
    for (int i = 0; i < 4; ++i) {
        const SegStage& g = p->st[i];
        const int C = SEG_DIMS[i], sr = SEG_SR[i];
        const size_t T = s.T[i], Tk = sr > 1 ? s.Tk[i] : T;
        int K;
        if (i == 0) {
            SEG_TRY(seg_gather_rgb(frame, chw, s, col, st));
            K = 147;
        } else {
            SEG_TRY(seg_im2col(ws + s.xs[i - 1], s.h[i - 1], s.w[i - 1], SEG_DIMS[i - 1], 3, 2, 1, s.h[i], s.w[i], col, st));
            K = 9 * SEG_DIMS[i - 1];
        }
        SEG_TRY(seg_gemm(col, g.pew, g.peb, nullptr, x, T, C, K, st));
        SEG_TRY(seg_ln(x, g.penw, g.penb, x, T, C, 1e-5f, st));
        for (const SegBlock& b : g.blocks) {
            SEG_TRY(seg_ln(x, b.n1w, b.n1b, xn, T, C, 1e-6f, st));
            SEG_TRY(seg_gemm(xn, b.qw, b.qb, nullptr, q, T, C, C, st));
            if (sr > 1) {
                SEG_TRY(seg_im2col(xn, s.h[i], s.w[i], C, sr, sr, 0, s.hk[i], s.wk[i], col, st));
                SEG_TRY(seg_gemm(col, b.srw, b.srb, nullptr, srb, Tk, C, sr * sr * C, st));
                SEG_TRY(seg_ln(srb, b.snw, b.snb, srb, Tk, C, 1e-5f, st));
                SEG_TRY(seg_gemm(srb, b.kvw, b.kvb, nullptr, kv, Tk, 2 * C, C, st));
            } else {
                SEG_TRY(seg_gemm(xn, b.kvw, b.kvb, nullptr, kv, Tk, 2 * C, C, st));
            }
            SEG_TRY(seg_attention(q, kv, xn, T, Tk, C, 0.125f, st));
            SEG_TRY(seg_gemm(xn, b.pw, b.pb, x, x, T, C, C, st));
            SEG_TRY(seg_ln(x, b.n2w, b.n2b, xn, T, C, 1e-6f, st));
            SEG_TRY(seg_gemm(xn, b.f1w, b.f1b, nullptr, h1, T, 4 * C, C, st));
            SEG_TRY(seg_dwconv_gelu(h1, b.dww, b.dwb, h2, s.h[i], s.w[i], 4 * C, st));
            SEG_TRY(seg_gemm(h2, b.f2w, b.f2b, x, x, T, C, 4 * C, st));
        }
        SEG_TRY(seg_ln(x, g.nw, g.nb, ws + s.xs[i], T, C, 1e-6f, st));
    }
    // decode head: one folded GEMM per scale at its own resolution, then upsample + sum + ReLU, then linear_pred
    HeadMaps mp;
    for (int i = 0; i < 4; ++i) {
        SEG_TRY(seg_gemm(ws + s.xs[i], p->fold[i], i == 0 ? p->foldb : nullptr, nullptr, ws + s.y[i], s.T[i], p->E, SEG_DIMS[i], st));
        mp.y[i] = ws + s.y[i]; mp.h[i] = s.h[i]; mp.w[i] = s.w[i];
    }
    SEG_TRY(seg_head_sum(mp, ws + s.y[0], p->E, st));
    SEG_TRY(seg_gemm(ws + s.y[0], p->predw, p->predb, nullptr, ws + s.lg, s.T[0], SEG_CLASSES, p->E, st));
    return VST_OK;
}

int seg_prepare(vst_seg* p, const void* frame, int H, int W, hipStream_t st, SegShape* s, float** ws) {
    if (!p || !frame) return VST_E_ARG;
    if (!seg_shape(H, W, s)) return VST_E_SHAPE;
    for (const SegTensor& t : p->tensors)
        if (!t.loaded) return VST_E_ARG;
    int dev = -1;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return (int)e;
    if (dev != p->device) return VST_E_ARG;
    seg_carve(s, p->E);
    return seg_arena(p, st, s->total, ws);
}

}  // namespace

extern "C" {

int vst_seg_create(const int* depths, int embed_dim, vst_seg** out) {
    if (!depths || !out) return VST_E_ARG;
    if (embed_dim < 4 || embed_dim > 2048 || (embed_dim & 3)) return VST_E_SHAPE;
    for (int i = 0; i < 4; ++i)
        if (depths[i] < 1 || depths[i] > 64) return VST_E_SHAPE;
    vst_seg* p = new vst_seg();
    hipError_t e = hipGetDevice(&p->device);
    if (e != hipSuccess) { delete p; return (int)e; }
    p->E = embed_dim;
    for (int i = 0; i < 4; ++i) {
        p->depths[i] = depths[i];
        p->st[i].blocks.resize(depths[i]);       // sized before any slot address is taken
    }
    for (int i = 0; i < 4; ++i) {
        SegStage& g = p->st[i];
        const size_t C = SEG_DIMS[i], sr = SEG_SR[i];
        const size_t Kpe = i == 0 ? 147 : 9 * (size_t)SEG_DIMS[i - 1];
        const std::string pe = "backbone.patch_embed" + std::to_string(i + 1) + ".";
        seg_register(p, pe + "proj.weight", C * Kpe, &g.pew);
        seg_register(p, pe + "proj.bias", C, &g.peb);
        seg_register(p, pe + "norm.weight", C, &g.penw);
        seg_register(p, pe + "norm.bias", C, &g.penb);
        for (int j = 0; j < depths[i]; ++j) {
            SegBlock& b = g.blocks[j];
            const std::string bk = "backbone.block" + std::to_string(i + 1) + "." + std::to_string(j) + ".";
            seg_register(p, bk + "norm1.weight", C, &b.n1w);
            seg_register(p, bk + "norm1.bias", C, &b.n1b);
            seg_register(p, bk + "attn.q.weight", C * C, &b.qw);
            seg_register(p, bk + "attn.q.bias", C, &b.qb);
            seg_register(p, bk + "attn.kv.weight", 2 * C * C, &b.kvw);
            seg_register(p, bk + "attn.kv.bias", 2 * C, &b.kvb);
            if (sr > 1) {
                seg_register(p, bk + "attn.sr.weight", C * sr * sr * C, &b.srw);
                seg_register(p, bk + "attn.sr.bias", C, &b.srb);
                seg_register(p, bk + "attn.norm.weight", C, &b.snw);
                seg_register(p, bk + "attn.norm.bias", C, &b.snb);
            } else {
                b.srw = b.srb = b.snw = b.snb = nullptr;
            }
            seg_register(p, bk + "attn.proj.weight", C * C, &b.pw);
            seg_register(p, bk + "attn.proj.bias", C, &b.pb);
            seg_register(p, bk + "norm2.weight", C, &b.n2w);
            seg_register(p, bk + "norm2.bias", C, &b.n2b);
            seg_register(p, bk + "mlp.fc1.weight", 4 * C * C, &b.f1w);
            seg_register(p, bk + "mlp.fc1.bias", 4 * C, &b.f1b);
            seg_register(p, bk + "mlp.dwconv.dwconv.weight", 9 * 4 * C, &b.dww);
            seg_register(p, bk + "mlp.dwconv.dwconv.bias", 4 * C, &b.dwb);
            seg_register(p, bk + "mlp.fc2.weight", 4 * C * C, &b.f2w);
            seg_register(p, bk + "mlp.fc2.bias", C, &b.f2b);
        }
        const std::string nm = "backbone.norm" + std::to_string(i + 1) + ".";
        seg_register(p, nm + "weight", C, &g.nw);
        seg_register(p, nm + "bias", C, &g.nb);
    }
    for (int i = 0; i < 4; ++i)
        seg_register(p, "decode_head.fold_c" + std::to_string(i + 1) + ".weight", (size_t)embed_dim * SEG_DIMS[i], &p->fold[i]);
    seg_register(p, "decode_head.fold.bias", embed_dim, &p->foldb);
    seg_register(p, "decode_head.linear_pred.weight", (size_t)SEG_CLASSES * embed_dim, &p->predw);
    seg_register(p, "decode_head.linear_pred.bias", SEG_CLASSES, &p->predb);
    size_t at = 0;
    for (SegTensor& t : p->tensors) { t.offset = at; at += (t.count + 63) / 64 * 64; }
    e = hipMalloc(&p->weights, at * sizeof(float));
    if (e != hipSuccess) { delete p; return (int)e; }
    for (SegTensor& t : p->tensors) *t.slot = p->weights + t.offset;
    *out = p;
    return VST_OK;
}

int vst_seg_tensor_count(const vst_seg* p) { return p ? (int)p->tensors.size() : VST_E_ARG; }

int vst_seg_tensor_info(const vst_seg* p, int i, const char** name, size_t* count) {
    if (!p || i < 0 || i >= (int)p->tensors.size() || !name || !count) return VST_E_ARG;
    *name = p->tensors[i].name.c_str();
    *count = p->tensors[i].count;
    return VST_OK;
}

int vst_seg_load_tensor(vst_seg* p, const char* name, const float* data_host, size_t count) {
    if (!p || !name || !data_host) return VST_E_ARG;
    const auto it = p->index.find(name);
    if (it == p->index.end()) return VST_E_ARG;
    SegTensor& t = p->tensors[it->second];
    if (t.count != count) return VST_E_SHAPE;
    hipError_t e = hipMemcpy(p->weights + t.offset, data_host, count * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) return (int)e;
    t.loaded = true;
    return VST_OK;
}

int vst_seg_run_scaled_u8(vst_seg* p, const uint8_t* work_u8, int chw, int Hw, int Ww, int H, int W, uint8_t* labels_u8,
                          void* stream) {
    if (!labels_u8) return VST_E_ARG;
    if (H < 1 || W < 1 || (int64_t)H * W > SEG_MAX_LABEL_PIXELS) return VST_E_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    SegShape s;
    float* ws = nullptr;
    SEG_TRY(seg_prepare(p, work_u8, Hw, Ww, st, &s, &ws));
    SEG_TRY(seg_forward(p, work_u8, chw, s, ws, st));
    return seg_labels(ws + s.lg, s.h[0], s.w[0], H, W, -1, labels_u8, st);
}

int vst_seg_run_u8(vst_seg* p, const uint8_t* frame_u8, int chw, int H, int W, uint8_t* labels_u8, void* stream) {
    return vst_seg_run_scaled_u8(p, frame_u8, chw, H, W, H, W, labels_u8, stream);
}

int vst_seg_labels_from_logits(const float* logits, int Hq, int Wq, int H, int W, int kernel, uint8_t* labels, void* stream) {
    if (!logits || !labels || ((uintptr_t)logits & 7)) return VST_E_ARG;
    if (Hq < 1 || Wq < 1 || (int64_t)Hq * Wq > SEG_MAX_LOGIT_CELLS || H < 1 || W < 1 || (int64_t)H * W > SEG_MAX_LABEL_PIXELS)
        return VST_E_SHAPE;
    return seg_labels(logits, Hq, Wq, H, W, kernel, labels, (hipStream_t)stream);
}

int vst_seg_mix_logits(const float* const* logits_host_array, const float* weights_host, int n, size_t count, float* out,
                       void* stream) {
    if (!logits_host_array || !weights_host || !out || ((uintptr_t)out & 7)) return VST_E_ARG;
    if (n < 1 || n > SEG_MIX_MAX || count == 0 || (count & 1) || count > (size_t)SEG_MAX_LOGIT_CELLS * SEG_CLASSES)
        return VST_E_SHAPE;
    SegMixArgs a;
    const uintptr_t o0 = (uintptr_t)out, bytes = count * sizeof(float);
    bool wide = (o0 & 15) == 0;
    for (int k = 0; k < SEG_MIX_MAX; ++k) {
        a.x[k] = k < n ? logits_host_array[k] : nullptr;
        a.w[k] = k < n ? weights_host[k] : 0.f;
        if (k >= n) continue;
        const uintptr_t x0 = (uintptr_t)a.x[k];
        if (!x0 || (x0 & 7)) return VST_E_ARG;
        if (x0 < o0 + bytes && o0 < x0 + bytes) return VST_E_ARG;      // out overlaps an input
        wide = wide && (x0 & 15) == 0;
    }
    hipStream_t st = (hipStream_t)stream;
    vst_prof_scope prof(VST_KERNEL_SEG_MIX, st);
    switch (n) {
        case 1: seg_mix_launch<1>(a, count, out, wide, st); break;
        case 2: seg_mix_launch<2>(a, count, out, wide, st); break;
        case 3: seg_mix_launch<3>(a, count, out, wide, st); break;
        case 4: seg_mix_launch<4>(a, count, out, wide, st); break;
        case 5: seg_mix_launch<5>(a, count, out, wide, st); break;
        case 6: seg_mix_launch<6>(a, count, out, wide, st); break;
        case 7: seg_mix_launch<7>(a, count, out, wide, st); break;
        default: seg_mix_launch<8>(a, count, out, wide, st); break;
    }
    VST_RETURN_IF_LAUNCH_FAILED();
    return VST_OK;
}

int vst_seg_logits(vst_seg* p, const uint8_t* frame_u8, int chw, int H, int W, float* logits, float* x1, float* x2, float* x3,
                   float* x4, void* stream) {
    if (!logits) return VST_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    SegShape s;
    float* ws = nullptr;
    SEG_TRY(seg_prepare(p, frame_u8, H, W, st, &s, &ws));
    SEG_TRY(seg_forward(p, frame_u8, chw, s, ws, st));
    hipError_t e = hipMemcpyAsync(logits, ws + s.lg, s.T[0] * SEG_CLASSES * sizeof(float), hipMemcpyDeviceToDevice, st);
    if (e != hipSuccess) return (int)e;
    float* xs[4] = {x1, x2, x3, x4};
    for (int i = 0; i < 4; ++i) {
        if (!xs[i]) continue;
        e = hipMemcpyAsync(xs[i], ws + s.xs[i], s.T[i] * SEG_DIMS[i] * sizeof(float), hipMemcpyDeviceToDevice, st);
        if (e != hipSuccess) return (int)e;
    }
    return VST_OK;
}

int vst_seg_shape(int H, int W, int* hw8) {
    SegShape s;
    if (!hw8) return VST_E_ARG;
    if (!seg_shape(H, W, &s)) return VST_E_SHAPE;
    for (int i = 0; i < 4; ++i) { hw8[2 * i] = s.h[i]; hw8[2 * i + 1] = s.w[i]; }
    return VST_OK;
}

// ---- kernel-level calls (tests and tools): the argument checks, then the launch helper seg_forward uses -------------------
namespace {
inline bool seg_f4(const void* p) { return p && ((uintptr_t)p & 15) == 0; }              // a float4-addressable pointer
inline bool seg_f4_or_null(const void* p) { return ((uintptr_t)p & 15) == 0; }
constexpr int64_t SEG_OP_MAX_FLOATS = (int64_t)1 << 30;                                   // per operand of a kernel-level call
}  // namespace

int vst_seg_gemm(const float* A, const float* W, const float* bias, const float* res, float* out, int M, int N, int K,
                 void* stream) {
    if (!seg_f4(A) || !seg_f4(W) || !seg_f4(out) || !seg_f4_or_null(bias) || !seg_f4_or_null(res)) return VST_E_ARG;
    if (M < 1 || N < 1 || K < 1 || (int64_t)M * K > SEG_OP_MAX_FLOATS || (int64_t)N * K > SEG_OP_MAX_FLOATS ||
        (int64_t)M * N > SEG_OP_MAX_FLOATS || (N + G_TILE - 1) / G_TILE > 65535)
        return VST_E_SHAPE;
    return seg_gemm(A, W, bias, res, out, (size_t)M, N, K, (hipStream_t)stream);
}

int vst_seg_layernorm(const float* x, const float* g, const float* b, float* out, int T, int C, float eps, void* stream) {
    if (!seg_f4(x) || !seg_f4(g) || !seg_f4(b) || !seg_f4(out)) return VST_E_ARG;
    if (T < 1 || C < 1 || C > SEG_MAX_C || (int64_t)T * C > SEG_OP_MAX_FLOATS) return VST_E_SHAPE;
    return seg_ln(x, g, b, out, (size_t)T, C, eps, (hipStream_t)stream);
}

int vst_seg_attention(const float* q, const float* kv, float* out, int N, int Nk, int C, float scale, void* stream) {
    if (!seg_f4(q) || !seg_f4(kv) || !seg_f4(out)) return VST_E_ARG;
    if (N < 1 || Nk < 1 || C < SEG_HEAD_DIM || C > SEG_MAX_C || C % SEG_HEAD_DIM) return VST_E_SHAPE;
    if ((int64_t)N * C > SEG_OP_MAX_FLOATS || (int64_t)Nk * 2 * C > SEG_OP_MAX_FLOATS) return VST_E_SHAPE;
    return seg_attention(q, kv, out, (size_t)N, (size_t)Nk, C, scale, (hipStream_t)stream);
}

int vst_seg_dwconv_gelu(const float* in, const float* w, const float* b, float* out, int H, int W, int C, void* stream) {
    if (!seg_f4(in) || !seg_f4(w) || !seg_f4(b) || !seg_f4(out)) return VST_E_ARG;
    if (H < 1 || W < 1 || C < 4 || (C & 3) || (int64_t)H * W * C > SEG_OP_MAX_FLOATS) return VST_E_SHAPE;
    return seg_dwconv_gelu(in, w, b, out, H, W, C, (hipStream_t)stream);
}

int vst_seg_im2col(const float* in, int Hi, int Wi, int C, int k, int stride, int pad, float* col, void* stream) {
    if (!seg_f4(in) || !seg_f4(col)) return VST_E_ARG;
    if (Hi < 1 || Wi < 1 || C < 4 || (C & 3) || k < 1 || k > 64 || stride < 1 || pad < 0 || pad >= k) return VST_E_SHAPE;
    if ((int64_t)Hi + 2 * pad < k || (int64_t)Wi + 2 * pad < k) return VST_E_SHAPE;
    const int Ho = (Hi + 2 * pad - k) / stride + 1, Wo = (Wi + 2 * pad - k) / stride + 1;
    if ((int64_t)Hi * Wi * C > SEG_OP_MAX_FLOATS || (int64_t)Ho * Wo * k * k * C > SEG_OP_MAX_FLOATS) return VST_E_SHAPE;
    return seg_im2col(in, Hi, Wi, C, k, stride, pad, Ho, Wo, col, (hipStream_t)stream);
}

int vst_seg_gather_rgb(const uint8_t* frame_u8, int chw, int H, int W, float* col, void* stream) {
    if (!frame_u8 || !seg_f4(col) || (chw != 0 && chw != 1)) return VST_E_ARG;
    SegShape s;
    if (!seg_shape(H, W, &s)) return VST_E_SHAPE;
    return seg_gather_rgb(frame_u8, chw, s, col, (hipStream_t)stream);
}

int vst_seg_head_sum(const float* y0, const float* y1, const float* y2, const float* y3, const int* hw8, int E, float* out,
                     void* stream) {
    if (!seg_f4(y0) || !seg_f4(y1) || !seg_f4(y2) || !seg_f4(y3) || !hw8 || !seg_f4(out)) return VST_E_ARG;
    if (E < 4 || (E & 3)) return VST_E_SHAPE;
    HeadMaps mp;
    const float* y[4] = {y0, y1, y2, y3};
    for (int i = 0; i < 4; ++i) {
        mp.y[i] = y[i]; mp.h[i] = hw8[2 * i]; mp.w[i] = hw8[2 * i + 1];
        if (mp.h[i] < 1 || mp.w[i] < 1 || (int64_t)mp.h[i] * mp.w[i] * E > SEG_OP_MAX_FLOATS) return VST_E_SHAPE;
    }
    return seg_head_sum(mp, out, E, (hipStream_t)stream);
}

int vst_seg_destroy(vst_seg* p) {
    if (!p) return VST_E_ARG;
    for (auto& kv : p->arenas)
        if (kv.second.base) (void)hipFree(kv.second.base);
    if (p->weights) (void)hipFree(p->weights);
    delete p;
    return VST_OK;
}

}  // extern "C"
