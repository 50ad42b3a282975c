// A frame's style map made on the device (vstnet.h, "Style maps per frame", version 120): from the frame's 8-bit weight planes
// to the two forms the mix reads - `dense` (K planes in image order, vst_cwct_mix_acc) and `rows` (K planes in the packed code's
// row order, vst_map_to_code) - in one launch on the frame's stream.  Pointwise and memory-bound.
#include "common.h"

namespace {

#define STYLE_FRAME_MAX_PLANES 8

__device__ __forceinline__ unsigned byte_of(unsigned dword, int x) { return (dword >> (8 * x)) & 255u; }

// Pillow's BOX 2 x 2 on 8-bit data, code pixel (i, j) of a cell whose four dword rows are v[0..3]: two rounded passes,
// horizontal first (strength_frame_kernel's)
__device__ __forceinline__ unsigned box_of(const unsigned (&v)[4], int i, int j) {
    const unsigned ht = (byte_of(v[2 * i], 2 * j) + byte_of(v[2 * i], 2 * j + 1) + 1u) >> 1;
    const unsigned hb = (byte_of(v[2 * i + 1], 2 * j) + byte_of(v[2 * i + 1], 2 * j + 1) + 1u) >> 1;
    return (ht + hb + 1u) >> 1;
}

// One thread per 4 x 4 pixel cell (h, w) of the frame, as in strength_frame_kernel: it loads the cell's four dword rows of every
// plane once (consecutive threads read consecutive dwords; 32 dwords at P = 8) and owns everything the cell produces, plane after
// plane, in that kernel's layout: SP = 2 four float4 of dense and two float4 per half of rows, SP = 1 one float2 of each per i.
// P is a run-time argument: every loop over planes is unrolled to 8 and predicated on the (wave-uniform) k < P, so the arrays are
// indexed by constants and stay in registers.  The arithmetic is the header's, operation for operation (no contraction).
template <int SP>
__global__ __launch_bounds__(256) void style_frame_kernel(const uint8_t* __restrict__ planes, int P, float* __restrict__ dense,
                                                          float* __restrict__ rows, int* __restrict__ flags, int H, int W) {
#pragma clang fp contract(off)
    const int Hq = H >> 2, Wq = W >> 2;
    const long cells = (long)Hq * Wq;
    const long c = (long)blockIdx.x * 256 + threadIdx.x;
    if (c >= cells) return;
    const int h = (int)(c / Wq), w = (int)(c - (long)h * Wq);
    const size_t frame = (size_t)H * W;                     // bytes of one plane
    constexpr int G = SP == 2 ? 4 : 2;                      // the cell's code pixels: G x G
    const size_t n = frame / (SP == 2 ? 1 : 4);             // floats of one output plane, dense and rows alike
    unsigned v[STYLE_FRAME_MAX_PLANES][4];                  // the cell's bytes: [plane][row], four columns per dword
#pragma unroll
    for (int k = 0; k < STYLE_FRAME_MAX_PLANES; ++k)
#pragma unroll
        for (int r = 0; r < 4; ++r)
            v[k][r] = k < P ? *(const unsigned*)(planes + (size_t)k * frame + (size_t)(4 * h + r) * W + 4 * (size_t)w) : 0u;
    // the code pixel (a, b) of plane k, after the reduction to the code grid
    auto u_of = [&](int k, int a, int b) -> unsigned { return SP == 2 ? byte_of(v[k][a], b) : box_of(v[k], a, b); };
    float total[G][G];                                       // (P >= 2) the planes' sum, exact in fp32: at most 8 * 255
    unsigned zero = 0;                                       // bit a * G + b: every plane is 0 at that code pixel
    if (P > 1) {
#pragma unroll
        for (int a = 0; a < G; ++a)
#pragma unroll
            for (int b = 0; b < G; ++b) {
                unsigned t = 0;
#pragma unroll
                for (int k = 0; k < STYLE_FRAME_MAX_PLANES; ++k)
                    if (k < P) t += u_of(k, a, b);
                total[a][b] = (float)t;
                if (t == 0) zero |= 1u << (a * G + b);
            }
    }
    const int K = P == 1 ? 2 : P;
#pragma unroll
    for (int k = 0; k < STYLE_FRAME_MAX_PLANES; ++k) {
        if (k >= K) continue;                                // (wave-uniform)
        float s[G][G];
#pragma unroll
        for (int a = 0; a < G; ++a)
#pragma unroll
            for (int b = 0; b < G; ++b) {
                if (P == 1) {                                // the ramp between two styles: (1 - t, t)
                    const float t = (float)u_of(0, a, b) / 255.0f;
                    s[a][b] = k == 0 ? 1.0f - t : t;
                } else {
                    const float q = (float)u_of(k, a, b) / total[a][b];
                    s[a][b] = (zero >> (a * G + b)) & 1u ? (k == 0 ? 1.0f : 0.0f) : q;
                }
            }
        float* dk = dense ? dense + (size_t)k * n : nullptr;
        float* rk = rows ? rows + (size_t)k * n : nullptr;
        if (SP == 2) {
            if (dk) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    *(float4*)(dk + (size_t)(4 * h + r) * W + 4 * (size_t)w) = make_float4(s[r][0], s[r][1], s[r][2], s[r][3]);
            }
            if (rk) {
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    float* d = rk + ((size_t)i * cells + (size_t)c) * 8;
                    *(float4*)d = make_float4(s[2 * i][0], s[2 * i][1], s[2 * i + 1][0], s[2 * i + 1][1]);
                    *(float4*)(d + 4) = make_float4(s[2 * i][2], s[2 * i][3], s[2 * i + 1][2], s[2 * i + 1][3]);
                }
            }
        } else {
            const int cW = W >> 1;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                if (dk) *(float2*)(dk + (size_t)(2 * h + i) * cW + 2 * (size_t)w) = make_float2(s[i][0], s[i][1]);
                if (rk) *(float2*)(rk + ((size_t)i * cells + (size_t)c) * 2) = make_float2(s[i][0], s[i][1]);
            }
        }
    }
    // one vector atomic per wave that saw a pixel no plane covers, issued by its first such lane; a clean frame issues none
    const unsigned long long saw = __ballot(zero != 0);
    if (flags && saw != 0 && (int)(threadIdx.x & 63) == __ffsll((long long)saw) - 1) atomicOr(flags, 1);
}

}  // namespace

int vst_style_frame(const uint8_t* planes, int n_planes, float* dense, float* rows, int* flags, int H, int W, int sp_steps,
                    void* stream) {
    if (!planes || (!dense && !rows) || n_planes < 1 || n_planes > STYLE_FRAME_MAX_PLANES) return VST_E_ARG;
    // dword loads of the byte planes, a dword atomic on the flag word, 16-byte stores of the float planes
    if ((((uintptr_t)planes | (uintptr_t)flags) & 3) || (((uintptr_t)dense | (uintptr_t)rows) & 15)) return VST_E_ARG;
    if (!vst_shape_ok(1, H, W)) return VST_E_SHAPE;
    if (sp_steps != 1 && sp_steps != 2) return VST_E_MODE;
    const long cells = (long)(H >> 2) * (W >> 2);
    const unsigned blocks = (unsigned)((cells + 255) / 256);         // at most 2^26 / 16 / 256 = 16384
    hipStream_t st = (hipStream_t)stream;
    if (sp_steps == 2) style_frame_kernel<2><<<blocks, 256, 0, st>>>(planes, n_planes, dense, rows, flags, H, W);
    else style_frame_kernel<1><<<blocks, 256, 0, st>>>(planes, n_planes, dense, rows, flags, H, W);
    VST_RETURN_IF_LAUNCH_FAILED();
    return VST_OK;
}
