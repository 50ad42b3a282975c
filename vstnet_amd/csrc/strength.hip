// A frame's strength map made on the device (vstnet.h, "Strength maps", version 110): from the frame's 8-bit matte and / or its
// label map and a 256-entry strength table to the two forms the blend reads - `dense` (image order, vst_cwct_blend) and `rows`
// (the packed code's row order, vst_map_to_code) - in one launch on the frame's stream.  Pointwise and memory-bound.
#include "common.h"

namespace {

// One thread per 4 x 4 pixel cell (h, w) of the frame: it loads the cell's four dword rows of matte and of labels (consecutive
// threads read consecutive dwords) and owns everything the cell produces.
//   SP = 2 (code grid = frame grid): 16 dense values as four float4 (row 4h + r, columns 4w .. 4w + 3) and, per half i, the
//           cell's 8 rows (g = 4j + 2i' + j' <-> pixel (4h + 2i + i', 4w + 2j + j'), mask_to_code_kernel's mapping) as two
//           float4: a wave writes 2 KiB without a gap per half.
//   SP = 1 (code grid = H/2 x W/2): the cell's 2 x 2 code pixels (2h + i, 2w + j): per i one float2 of dense and one of rows.
// The arithmetic is the header's, operation for operation (no contraction): a test restates it bit for bit.
template <int SP>
__global__ __launch_bounds__(256) void strength_frame_kernel(const uint8_t* __restrict__ matte, const uint8_t* __restrict__ labels,
                                                             const float* __restrict__ table, float* __restrict__ dense,
                                                             float* __restrict__ rows, int H, int W) {
#pragma clang fp contract(off)
    __shared__ float tab[256];
    if (labels) tab[threadIdx.x] = table[threadIdx.x];
    __syncthreads();
    const int Hq = H >> 2, Wq = W >> 2;
    const long cells = (long)Hq * Wq;
    const long c = (long)blockIdx.x * 256 + threadIdx.x;
    if (c >= cells) return;
    const int h = (int)(c / Wq), w = (int)(c - (long)h * Wq);
    unsigned mv[4][4], lv[4][4];                           // the cell's bytes, [row][column]
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const size_t off = (size_t)(4 * h + r) * W + 4 * (size_t)w;
        const unsigned mw = matte ? *(const unsigned*)(matte + off) : 0u;
        const unsigned lw = labels ? *(const unsigned*)(labels + off) : 0u;
#pragma unroll
        for (int x = 0; x < 4; ++x) {
            mv[r][x] = (mw >> (8 * x)) & 255u;
            lv[r][x] = (lw >> (8 * x)) & 255u;
        }
    }
    if (SP == 2) {
        float s[4][4];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int x = 0; x < 4; ++x) {
                const float m = (float)mv[r][x] / 255.0f;
                const float t = labels ? tab[lv[r][x]] : 1.0f;
                s[r][x] = !labels ? m : (!matte ? t : m * t);
            }
        if (dense) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                *(float4*)(dense + (size_t)(4 * h + r) * W + 4 * (size_t)w) = make_float4(s[r][0], s[r][1], s[r][2], s[r][3]);
        }
        if (rows) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                float* d = rows + ((size_t)i * cells + (size_t)c) * 8;
                *(float4*)d = make_float4(s[2 * i][0], s[2 * i][1], s[2 * i + 1][0], s[2 * i + 1][1]);
                *(float4*)(d + 4) = make_float4(s[2 * i][2], s[2 * i][3], s[2 * i + 1][2], s[2 * i + 1][3]);
            }
        }
    } else {
        float s[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                // Pillow's BOX 2 x 2 on 8-bit data: two rounded passes, horizontal first
                const unsigned ht = (mv[2 * i][2 * j] + mv[2 * i][2 * j + 1] + 1u) >> 1;
                const unsigned hb = (mv[2 * i + 1][2 * j] + mv[2 * i + 1][2 * j + 1] + 1u) >> 1;
                const float m = (float)((ht + hb + 1u) >> 1) / 255.0f;
                float t = 1.0f;
                if (labels) {
                    const float top = tab[lv[2 * i][2 * j]] + tab[lv[2 * i][2 * j + 1]];
                    const float bot = tab[lv[2 * i + 1][2 * j]] + tab[lv[2 * i + 1][2 * j + 1]];
                    t = (top + bot) * 0.25f;
                }
                s[i][j] = !labels ? m : (!matte ? t : m * t);
            }
        const int cW = W >> 1;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            if (dense) *(float2*)(dense + (size_t)(2 * h + i) * cW + 2 * (size_t)w) = make_float2(s[i][0], s[i][1]);
            if (rows) *(float2*)(rows + ((size_t)i * cells + (size_t)c) * 2) = make_float2(s[i][0], s[i][1]);
        }
    }
}

}  // namespace

int vst_strength_frame(const uint8_t* matte, const uint8_t* labels, const float* table, float* dense, float* rows, int H, int W,
                       int sp_steps, void* stream) {
    if ((!matte && !labels) || (!dense && !rows) || (labels && !table)) return VST_E_ARG;
    // dword loads of the byte maps, 16-byte stores of the float maps
    if ((((uintptr_t)matte | (uintptr_t)labels | (uintptr_t)table) & 3) || (((uintptr_t)dense | (uintptr_t)rows) & 15)) return VST_E_ARG;
    if (!vst_shape_ok(1, H, W)) return VST_E_SHAPE;
    if (sp_steps != 1 && sp_steps != 2) return VST_E_MODE;
    const long cells = (long)(H >> 2) * (W >> 2);
    const unsigned blocks = (unsigned)((cells + 255) / 256);         // at most 2^26 / 16 / 256 = 16384
    hipStream_t st = (hipStream_t)stream;
    if (sp_steps == 2) strength_frame_kernel<2><<<blocks, 256, 0, st>>>(matte, labels, table, dense, rows, H, W);
    else strength_frame_kernel<1><<<blocks, 256, 0, st>>>(matte, labels, table, dense, rows, H, W);
    VST_RETURN_IF_LAUNCH_FAILED();
    return VST_OK;
}
