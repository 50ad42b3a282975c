// The deep resize (vst_yuv16_img_resize_f32; DESIGN.md section 6, "Deep resize"): what resize.hip, which owns the entry point and
// the plain passes, and yuv.hip, which owns the pixel arithmetic and with it the fused first pass, share.
#pragma once
#include "common.h"

constexpr int DEEP_H_PIX = 64;                       // output columns of one workgroup of the fused pass
constexpr size_t DEEP_H_LDS_BYTES = 48 * 1024;       // its LDS budget: rows = budget / (3 channels * span * 4 B), 1..8

#ifdef __HIPCC__
// The last pass's epilogue: the accumulated value clamped to [0, 1] and rounded to fp32 into planes [3][H][W]; the u8 twin (HWC,
// if asked for) is floor(255 v + 0.5) of that STORED value v, evaluated in double - an exact function of the float output.
__device__ __forceinline__ float vst_deep_final_value(double acc) { return (float)fmin(fmax(acc, 0.0), 1.0); }
__device__ __forceinline__ uint8_t vst_deep_twin(float v) { return (uint8_t)floor(255.0 * (double)v + 0.5); }
__device__ __forceinline__ void vst_deep_final_store(float* __restrict__ out, uint8_t* __restrict__ out_u8, size_t plane, int W,
                                                     int c, int y, int x, double acc) {
    const float v = vst_deep_final_value(acc);
    const size_t px = (size_t)y * W + x;
    out[c * plane + px] = v;
    if (out_u8) out_u8[px * 3 + c] = vst_deep_twin(v);
}
#endif

// yuv.hip.  VST_E_ARG unless the planes, the size and (depth, layout, matrix, range) are what vst_yuv16_to_rgb_f32 takes
VST_INTERNAL int vst_deep_yuv_check(const void* y, const void* u, const void* v, int H, int W, int depth, int layout, int matrix,
                                    int range);
// the fused pass: planes of an H x W frame -> dst = float [3][H][Wd] with the table (W -> Wd, double weights, `ksize` of them per
// column) on the device; final != 0: dst is the frame's output, clamped, and dst_u8 (or NULL) its u8 twin
VST_INTERNAL int vst_deep_resize_h_fused(const uint16_t* y, const uint16_t* u, const uint16_t* v, int H, int W, int depth,
                                         int layout, int matrix, int range, const int* table, int Wd, int ksize, float* dst,
                                         uint8_t* dst_u8, int final, hipStream_t st);
