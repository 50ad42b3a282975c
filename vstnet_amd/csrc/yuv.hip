// Raw video edge: 8-bit Y'CbCr planes <-> the uint8 HWC RGB frame of the video loop (vstnet.h: vst_yuv_to_rgb_u8,
// vst_rgb_to_yuv_u8; the arithmetic is stated there and restated in float64 by vstnet_amd/yuv.py).
// Pointwise and launch-latency class: 4.5 B per pixel each way at 4:2:0.  One lane owns 4 consecutive luma pixels of a row
// (to RGB) or a 4 x 2 luma block and its two chroma samples (to 4:2:0): a dword of Y and three dwords of RGB per lane where the
// row's base is 4-byte aligned, consecutive lanes on consecutive addresses; rows whose base is not aligned (W mod 4 != 0) and
// the ragged right edge take guarded byte accesses.  Chroma neighbours are read as bytes (a quarter of the traffic, and the
// lanes' columns are adjacent): 8 per plane and lane on the way to RGB, shared by the lane's 4 pixels.  No LDS, no arrays
// indexed at run time.
#include "common.h"

namespace {

enum { AL_Y = 1, AL_RGB = 2, AL_UV = 4 };      // which pointers sit on the 4-byte grid (AL_UV, 4:2:0 to YUV: on the 2-byte grid)

struct ToRgb {          // R = ys (Y - yoff) + rv pr ..., with pb, pr = cs (C - 128)
    float yoff, ys, cs, rv, gu, gv, bu;
};
struct ToYuv {          // Y = kr R + kg G + kb B; Cb = icb (B - Y), Cr = icr (R - Y); bytes yoff + ysc Y, 128 + csc C
    float kr, kg, kb, icb, icr, yoff, ysc, csc;
};

__device__ __forceinline__ uint32_t round_u8(float v) {         // clamp(floor(v + 0.5), 0, 255)
    return (uint32_t)fminf(fmaxf(floorf(v + 0.5f), 0.0f), 255.0f);
}

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// Bilinear samples of a 4:2:0 plane at the 4 luma pixels (yl, x0 .. x0 + 3), x0 % 4 == 0.  The chroma coordinate of luma x is
// (x - 1/2) / 2 (centre) or x / 2 (left), of luma y (y - 1/2) / 2, so the 4 pixels read the chroma columns x0 / 2 - 1 .. x0 / 2 + 2
// of two rows: 8 bytes per plane, shared between the pixels, the rows blended first.  Indices are clamped to the plane (a lane
// at the ragged right edge reads clamped columns for the pixels it does not store).  Exact in fp32: the weights are multiples
// of 1/4 and the values bytes, so the order of the two blends changes nothing.
template <int LAYOUT>
__device__ __forceinline__ void chroma4(const uint8_t* __restrict__ p, int Hc, int Wc, int yl, int x0, float (&out)[4]) {
    // even rows sit 3/4 of the way from sample yl / 2 - 1 to yl / 2, odd rows 1/4 of the way from yl / 2 to yl / 2 + 1
    const int i0 = (yl >> 1) - ((yl & 1) ? 0 : 1);
    const float wy = (yl & 1) ? 0.25f : 0.75f;
    const uint8_t* ra = p + (size_t)clampi(i0, Hc - 1) * Wc;
    const uint8_t* rb = p + (size_t)clampi(i0 + 1, Hc - 1) * Wc;
    const int j0 = (x0 >> 1) - 1;
    float c[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int j = clampi(j0 + k, Wc - 1);
        c[k] = (1.0f - wy) * (float)ra[j] + wy * (float)rb[j];
    }
    if (LAYOUT == VST_YUV_420_CENTRE) {         // x0: 3/4 from c0 to c1; x0 + 1, + 2: 1/4 and 3/4 from c1 to c2; x0 + 3: 1/4 from c2 to c3
        out[0] = 0.25f * c[0] + 0.75f * c[1];
        out[1] = 0.75f * c[1] + 0.25f * c[2];
        out[2] = 0.25f * c[1] + 0.75f * c[2];
        out[3] = 0.75f * c[2] + 0.25f * c[3];
    } else {                                    // co-sited with the even columns: on c1, between c1 and c2, on c2, between c2 and c3
        out[0] = c[1];
        out[1] = 0.5f * c[1] + 0.5f * c[2];
        out[2] = c[2];
        out[3] = 0.5f * c[2] + 0.5f * c[3];
    }
}

template <int LAYOUT>
__global__ __launch_bounds__(256) void yuv_to_rgb_kernel(const uint8_t* __restrict__ yp, const uint8_t* __restrict__ up,
                                                         const uint8_t* __restrict__ vp, int H, int W, int quads, ToRgb k,
                                                         int al, uint8_t* __restrict__ rgb) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    const int row = idx / quads, x0 = (idx - row * quads) * 4;
    if (row >= H) return;
    const size_t base = (size_t)row * W + x0;
    const int n = min(4, W - x0);
    const bool on_grid = n == 4 && (base & 3) == 0;
    const int Hc = (H + 1) >> 1, Wc = (W + 1) >> 1;
    float Y[4], U[4], V[4];
    if (on_grid && (al & AL_Y)) {
        const uint32_t w = *reinterpret_cast<const uint32_t*>(yp + base);
#pragma unroll
        for (int p = 0; p < 4; ++p) Y[p] = (float)((w >> (8 * p)) & 0xffu);
    } else {
#pragma unroll
        for (int p = 0; p < 4; ++p) Y[p] = p < n ? (float)yp[base + p] : 0.0f;
    }
    if (LAYOUT == VST_YUV_444) {
        if (on_grid && (al & AL_UV)) {
            const uint32_t wu = *reinterpret_cast<const uint32_t*>(up + base), wv = *reinterpret_cast<const uint32_t*>(vp + base);
#pragma unroll
            for (int p = 0; p < 4; ++p) U[p] = (float)((wu >> (8 * p)) & 0xffu), V[p] = (float)((wv >> (8 * p)) & 0xffu);
        } else {
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                U[p] = p < n ? (float)up[base + p] : 128.0f;
                V[p] = p < n ? (float)vp[base + p] : 128.0f;
            }
        }
    } else {
        chroma4<LAYOUT>(up, Hc, Wc, row, x0, U);
        chroma4<LAYOUT>(vp, Hc, Wc, row, x0, V);
    }
    uint32_t o[12];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const float yy = (Y[p] - k.yoff) * k.ys, pb = (U[p] - 128.0f) * k.cs, pr = (V[p] - 128.0f) * k.cs;
        o[3 * p + 0] = round_u8(yy + k.rv * pr);
        o[3 * p + 1] = round_u8(yy - k.gv * pr - k.gu * pb);
        o[3 * p + 2] = round_u8(yy + k.bu * pb);
    }
    uint8_t* dst = rgb + base * 3;
    if (on_grid && (al & AL_RGB)) {             // 3 * base is a multiple of 4 with base
        uint32_t* dw = reinterpret_cast<uint32_t*>(dst);
#pragma unroll
        for (int j = 0; j < 3; ++j) dw[j] = o[4 * j] | (o[4 * j + 1] << 8) | (o[4 * j + 2] << 16) | (o[4 * j + 3] << 24);
    } else {
#pragma unroll
        for (int p = 0; p < 4; ++p)
            if (p < n) dst[3 * p] = (uint8_t)o[3 * p], dst[3 * p + 1] = (uint8_t)o[3 * p + 1], dst[3 * p + 2] = (uint8_t)o[3 * p + 2];
    }
}

// 4 pixels of row `row` from column x0 (x0 % 4 == 0, x0 < W): columns past the right edge repeat the last one
__device__ __forceinline__ void load_rgb4(const uint8_t* __restrict__ rgb, int row, int x0, int W, bool rgb_aligned,
                                          float (&r)[4], float (&g)[4], float (&b)[4]) {
    const size_t base = (size_t)row * W + x0;
    if (x0 + 4 <= W && (base & 3) == 0 && rgb_aligned) {
        const uint32_t* sw = reinterpret_cast<const uint32_t*>(rgb + base * 3);
        const uint32_t w0 = sw[0], w1 = sw[1], w2 = sw[2];
        r[0] = (float)(w0 & 0xffu), g[0] = (float)((w0 >> 8) & 0xffu), b[0] = (float)((w0 >> 16) & 0xffu);
        r[1] = (float)(w0 >> 24), g[1] = (float)(w1 & 0xffu), b[1] = (float)((w1 >> 8) & 0xffu);
        r[2] = (float)((w1 >> 16) & 0xffu), g[2] = (float)(w1 >> 24), b[2] = (float)(w2 & 0xffu);
        r[3] = (float)((w2 >> 8) & 0xffu), g[3] = (float)((w2 >> 16) & 0xffu), b[3] = (float)(w2 >> 24);
    } else {
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const uint8_t* s = rgb + ((size_t)row * W + min(x0 + p, W - 1)) * 3;
            r[p] = (float)s[0], g[p] = (float)s[1], b[p] = (float)s[2];
        }
    }
}

// 4 bytes (values already rounded) to dst[0..n): one dword where the address allows
__device__ __forceinline__ void store4(uint8_t* dst, size_t off, int n, bool aligned, const uint32_t (&q)[4]) {
    if (n == 4 && (off & 3) == 0 && aligned) {
        *reinterpret_cast<uint32_t*>(dst + off) = q[0] | (q[1] << 8) | (q[2] << 16) | (q[3] << 24);
    } else {
#pragma unroll
        for (int p = 0; p < 4; ++p)
            if (p < n) dst[off + p] = (uint8_t)q[p];
    }
}

__global__ __launch_bounds__(256) void rgb_to_yuv444_kernel(const uint8_t* __restrict__ rgb, int H, int W, int quads, ToYuv k,
                                                            int al, uint8_t* __restrict__ yp, uint8_t* __restrict__ up,
                                                            uint8_t* __restrict__ vp) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    const int row = idx / quads, x0 = (idx - row * quads) * 4;
    if (row >= H) return;
    const int n = min(4, W - x0);
    float r[4], g[4], b[4];
    load_rgb4(rgb, row, x0, W, (al & AL_RGB) != 0, r, g, b);
    uint32_t qy[4], qu[4], qv[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const float Y = k.kr * r[p] + k.kg * g[p] + k.kb * b[p];
        qy[p] = round_u8(k.yoff + Y * k.ysc);
        qu[p] = round_u8(128.0f + (b[p] - Y) * k.icb * k.csc);
        qv[p] = round_u8(128.0f + (r[p] - Y) * k.icr * k.csc);
    }
    const size_t base = (size_t)row * W + x0;
    store4(yp, base, n, (al & AL_Y) != 0, qy);
    store4(up, base, n, (al & AL_UV) != 0, qu);
    store4(vp, base, n, (al & AL_UV) != 0, qv);
}

// one lane: luma rows 2i, 2i + 1, columns x0 .. x0 + 3 -> two dwords of Y, chroma samples (i, x0 / 2) and (i, x0 / 2 + 1)
template <int LAYOUT>
__global__ __launch_bounds__(256) void rgb_to_yuv420_kernel(const uint8_t* __restrict__ rgb, int H, int W, int quads, ToYuv k,
                                                            int al, uint8_t* __restrict__ yp, uint8_t* __restrict__ up,
                                                            uint8_t* __restrict__ vp) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    const int Hc = (H + 1) >> 1, Wc = (W + 1) >> 1;
    const int i = idx / quads, x0 = (idx - i * quads) * 4;
    if (i >= Hc) return;
    const int n = min(4, W - x0);
    float cb[2][5], cr[2][5];                   // [row of the pair][column x0 - 1 .. x0 + 3]; column 0 only for left siting
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
        const int row = min(2 * i + dy, H - 1);         // odd H: the last row again
        float r[4], g[4], b[4];
        load_rgb4(rgb, row, x0, W, (al & AL_RGB) != 0, r, g, b);
        uint32_t qy[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const float Y = k.kr * r[p] + k.kg * g[p] + k.kb * b[p];
            qy[p] = round_u8(k.yoff + Y * k.ysc);
            cb[dy][p + 1] = (b[p] - Y) * k.icb;
            cr[dy][p + 1] = (r[p] - Y) * k.icr;
        }
        if (2 * i + dy < H) store4(yp, (size_t)row * W + x0, n, (al & AL_Y) != 0, qy);
        if (LAYOUT == VST_YUV_420_LEFT) {       // the left neighbour column, re-read from memory (column 0: itself)
            const uint8_t* s = rgb + ((size_t)row * W + max(x0 - 1, 0)) * 3;
            const float rr = (float)s[0], gg = (float)s[1], bb = (float)s[2];
            const float Y = k.kr * rr + k.kg * gg + k.kb * bb;
            cb[dy][0] = (bb - Y) * k.icb;
            cr[dy][0] = (rr - Y) * k.icr;
        }
    }
    uint32_t qu[2], qv[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {               // chroma column x0 / 2 + j, luma columns x0 + 2 j (- 1), + 1 (load_rgb4 replicated)
        float fb, fr;
        if (LAYOUT == VST_YUV_420_CENTRE) {
            fb = 0.25f * ((cb[0][2 * j + 1] + cb[0][2 * j + 2]) + (cb[1][2 * j + 1] + cb[1][2 * j + 2]));
            fr = 0.25f * ((cr[0][2 * j + 1] + cr[0][2 * j + 2]) + (cr[1][2 * j + 1] + cr[1][2 * j + 2]));
        } else {
            fb = 0.5f * ((0.25f * cb[0][2 * j] + 0.5f * cb[0][2 * j + 1] + 0.25f * cb[0][2 * j + 2]) +
                         (0.25f * cb[1][2 * j] + 0.5f * cb[1][2 * j + 1] + 0.25f * cb[1][2 * j + 2]));
            fr = 0.5f * ((0.25f * cr[0][2 * j] + 0.5f * cr[0][2 * j + 1] + 0.25f * cr[0][2 * j + 2]) +
                         (0.25f * cr[1][2 * j] + 0.5f * cr[1][2 * j + 1] + 0.25f * cr[1][2 * j + 2]));
        }
        qu[j] = round_u8(128.0f + fb * k.csc);
        qv[j] = round_u8(128.0f + fr * k.csc);
    }
    const int jc = x0 >> 1;
    const size_t off = (size_t)i * Wc + jc;
    if (jc + 1 < Wc && (off & 1) == 0 && (al & AL_UV)) {
        *reinterpret_cast<uint16_t*>(up + off) = (uint16_t)(qu[0] | (qu[1] << 8));
        *reinterpret_cast<uint16_t*>(vp + off) = (uint16_t)(qv[0] | (qv[1] << 8));
    } else {
        up[off] = (uint8_t)qu[0], vp[off] = (uint8_t)qv[0];
        if (jc + 1 < Wc) up[off + 1] = (uint8_t)qu[1], vp[off + 1] = (uint8_t)qv[1];
    }
}

bool yuv_coefficients(int matrix, int range, double& kr, double& kb, double& yoff, double& ys, double& cs) {
    if (matrix == VST_YUV_BT601) kr = 0.299, kb = 0.114;
    else if (matrix == VST_YUV_BT709) kr = 0.2126, kb = 0.0722;
    else return false;
    if (range == VST_YUV_LIMITED) yoff = 16.0, ys = 219.0, cs = 224.0;
    else if (range == VST_YUV_FULL) yoff = 0.0, ys = 255.0, cs = 255.0;
    else return false;
    return true;
}

bool yuv_args_ok(const void* a, const void* b, const void* c, const void* d, int H, int W, int layout) {
    return a && b && c && d && H >= 1 && W >= 1 && (int64_t)H * W <= VST_MAX_FRAME_PIXELS &&
           (layout == VST_YUV_444 || layout == VST_YUV_420_CENTRE || layout == VST_YUV_420_LEFT);
}

}  // namespace

extern "C" int vst_yuv_to_rgb_u8(const uint8_t* y, const uint8_t* u, const uint8_t* v, int H, int W, int layout, int matrix,
                                 int range, uint8_t* rgb_hwc, void* stream) {
    double kr, kb, yoff, ys, cs;
    if (!yuv_args_ok(y, u, v, rgb_hwc, H, W, layout) || !yuv_coefficients(matrix, range, kr, kb, yoff, ys, cs)) return VST_E_ARG;
    const double kg = 1.0 - kr - kb;
    ToRgb k;
    k.yoff = (float)yoff, k.ys = (float)(255.0 / ys), k.cs = (float)(255.0 / cs);
    k.rv = (float)(2.0 * (1.0 - kr)), k.bu = (float)(2.0 * (1.0 - kb));
    k.gv = (float)(2.0 * (1.0 - kr) * kr / kg), k.gu = (float)(2.0 * (1.0 - kb) * kb / kg);
    const int al = (((uintptr_t)y & 3) == 0 ? AL_Y : 0) | (((uintptr_t)rgb_hwc & 3) == 0 ? AL_RGB : 0) |
                   ((((uintptr_t)u | (uintptr_t)v) & 3) == 0 ? AL_UV : 0);
    const int quads = (W + 3) / 4;
    const unsigned blocks = (unsigned)(((int64_t)quads * H + 255) / 256);
    hipStream_t st = (hipStream_t)stream;
    if (layout == VST_YUV_444)
        yuv_to_rgb_kernel<VST_YUV_444><<<blocks, 256, 0, st>>>(y, u, v, H, W, quads, k, al, rgb_hwc);
    else if (layout == VST_YUV_420_CENTRE)
        yuv_to_rgb_kernel<VST_YUV_420_CENTRE><<<blocks, 256, 0, st>>>(y, u, v, H, W, quads, k, al, rgb_hwc);
    else
        yuv_to_rgb_kernel<VST_YUV_420_LEFT><<<blocks, 256, 0, st>>>(y, u, v, H, W, quads, k, al, rgb_hwc);
    VST_RETURN_IF_LAUNCH_FAILED();
    return VST_OK;
}

extern "C" int vst_rgb_to_yuv_u8(const uint8_t* rgb_hwc, int H, int W, int layout, int matrix, int range, uint8_t* y,
                                 uint8_t* u, uint8_t* v, void* stream) {
    double kr, kb, yoff, ys, cs;
    if (!yuv_args_ok(y, u, v, rgb_hwc, H, W, layout) || !yuv_coefficients(matrix, range, kr, kb, yoff, ys, cs)) return VST_E_ARG;
    ToYuv k;
    k.kr = (float)kr, k.kb = (float)kb, k.kg = (float)(1.0 - kr - kb);
    k.icb = (float)(1.0 / (2.0 * (1.0 - kb))), k.icr = (float)(1.0 / (2.0 * (1.0 - kr)));
    k.yoff = (float)yoff, k.ysc = (float)(ys / 255.0), k.csc = (float)(cs / 255.0);
    const int uv_grid = layout == VST_YUV_444 ? 3 : 1;
    const int al = (((uintptr_t)y & 3) == 0 ? AL_Y : 0) | (((uintptr_t)rgb_hwc & 3) == 0 ? AL_RGB : 0) |
                   ((((uintptr_t)u | (uintptr_t)v) & uv_grid) == 0 ? AL_UV : 0);
    const int quads = (W + 3) / 4;
    const int rows = layout == VST_YUV_444 ? H : (H + 1) / 2;
    const unsigned blocks = (unsigned)(((int64_t)quads * rows + 255) / 256);
    hipStream_t st = (hipStream_t)stream;
    if (layout == VST_YUV_444)
        rgb_to_yuv444_kernel<<<blocks, 256, 0, st>>>(rgb_hwc, H, W, quads, k, al, y, u, v);
    else if (layout == VST_YUV_420_CENTRE)
        rgb_to_yuv420_kernel<VST_YUV_420_CENTRE><<<blocks, 256, 0, st>>>(rgb_hwc, H, W, quads, k, al, y, u, v);
    else
        rgb_to_yuv420_kernel<VST_YUV_420_LEFT><<<blocks, 256, 0, st>>>(rgb_hwc, H, W, quads, k, al, y, u, v);
    VST_RETURN_IF_LAUNCH_FAILED();
    return VST_OK;
}
