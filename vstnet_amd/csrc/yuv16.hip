// High-bit-depth edge: 9..16-bit Y'CbCr planes (little-endian 16-bit samples) <-> fp32 RGB planes [3][H][W] on a 0..1 scale
// (vstnet.h: vst_yuv16_to_rgb_f32, vst_rgb_f32_to_yuv16; the arithmetic is stated there and restated in float64 by
// vstnet_amd/yuv16.py).  Built next to yuv.hip, which it follows in shape and leaves alone.
// Arithmetic: fp64 per pixel, one rounding at the end (to a code, to a byte of the u8 side output, or to fp32).  At depth 16 a
// code has magnitude 2^16, where fp32 leaves a quarter of a code of doubt at every rounding; in fp64 the few dozen operations of
// a pixel err by under 2^-32 of a code, so a code equals floor(v + 0.5) of the exact value unless v lies within 2^-20 of a tie.
// The kernels are pointwise and bound by their 18 to 30 bytes per pixel; the fp64 operations do not show next to that.
// One lane owns 4 consecutive luma pixels of a row (to RGB, to 4:4:4), a 4 x 2 luma block and its two chroma samples (to 4:2:0)
// or 4 pixels of a row and their two chroma samples (to 4:2:2): 8 bytes of Y, 16 bytes per fp32 plane and three dwords of the
// u8 output per lane where the ADDRESS is on that grid (checked per lane: a pointer needs 2-byte alignment and nothing more, and
// the planes of one flat Y|U|V buffer start wherever H and W put them), consecutive lanes on consecutive addresses; everything
// else - rows of a width that is no multiple of 4, the ragged right edge, bases off the grid - takes guarded narrow accesses.
// Chroma neighbours on the way to RGB are read as single samples, shared by the lane's 4 pixels.  No LDS, no arrays indexed at
// run time.
#include "common.h"

namespace {

struct ToRgb16 {        // y' = (min(Y, maxc) - yoff) iys, pb = (U - coff) ics, pr = (V - coff) ics; R = y' + rv pr ...
    double yoff, iys, coff, ics, rv, gu, gv, bu;
    uint32_t maxc;
};
struct ToYuv16 {        // Y = kr R + kg G + kb B; Cb = icb (B - Y), Cr = icr (R - Y); codes yoff + ys Y, coff + cs C
    double kr, kg, kb, icb, icr, yoff, ys, coff, cs, maxc;
};

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }
__device__ __forceinline__ double clamp01(double v) { return fmin(fmax(v, 0.0), 1.0); }
__device__ __forceinline__ uint32_t round_code(double v, double maxc) {        // clamp(floor(v + 0.5), 0, 2^depth - 1)
    return (uint32_t)fmin(fmax(floor(v + 0.5), 0.0), maxc);
}
__device__ __forceinline__ bool on_grid(const void* p, uintptr_t grid) { return ((uintptr_t)p & (grid - 1)) == 0; }

// 4 samples of row base p + off (n of them inside the plane), limited to maxc; `fill` stands in past the edge
__device__ __forceinline__ void load4_u16(const uint16_t* __restrict__ p, size_t off, int n, uint32_t maxc, double fill,
                                          double (&out)[4]) {
    if (n == 4 && on_grid(p + off, 8)) {
        const uint2 w = *reinterpret_cast<const uint2*>(p + off);
        out[0] = (double)min(w.x & 0xffffu, maxc), out[1] = (double)min(w.x >> 16, maxc);
        out[2] = (double)min(w.y & 0xffffu, maxc), out[3] = (double)min(w.y >> 16, maxc);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) out[k] = k < n ? (double)min((uint32_t)p[off + k], maxc) : fill;
    }
}

// Chroma of the 4 luma pixels (yl, x0 .. x0 + 3), x0 % 4 == 0, from a subsampled plane of Hc x Wc samples.  4:2:0: the taps of
// yuv.hip's chroma4 - the chroma coordinate of luma x is (x - 1/2) / 2 (centre) or x / 2 (left), of luma y (y - 1/2) / 2 - so
// the pixels read the columns x0 / 2 - 1 .. x0 / 2 + 2 of two rows.  4:2:2: the row itself, columns as for left siting.
// Indices are clamped to the plane.  The weights are multiples of 1/4 and the values integers: exact.
template <int LAYOUT>
__device__ __forceinline__ void chroma4(const uint16_t* __restrict__ p, int Hc, int Wc, int yl, int x0, uint32_t maxc,
                                        double (&out)[4]) {
    const int j0 = (x0 >> 1) - 1;
    double c[4];
    if (LAYOUT == VST_YUV_422) {
        const uint16_t* ra = p + (size_t)yl * Wc;
#pragma unroll
        for (int k = 0; k < 4; ++k) c[k] = (double)min((uint32_t)ra[clampi(j0 + k, Wc - 1)], maxc);
    } else {
        // even rows sit 3/4 of the way from sample yl / 2 - 1 to yl / 2, odd rows 1/4 of the way from yl / 2 to yl / 2 + 1
        const int i0 = (yl >> 1) - ((yl & 1) ? 0 : 1);
        const double wy = (yl & 1) ? 0.25 : 0.75;
        const uint16_t* ra = p + (size_t)clampi(i0, Hc - 1) * Wc;
        const uint16_t* rb = p + (size_t)clampi(i0 + 1, Hc - 1) * Wc;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int j = clampi(j0 + k, Wc - 1);
            c[k] = (1.0 - wy) * (double)min((uint32_t)ra[j], maxc) + wy * (double)min((uint32_t)rb[j], maxc);
        }
    }
    if (LAYOUT == VST_YUV_420_CENTRE) {
        out[0] = 0.25 * c[0] + 0.75 * c[1];
        out[1] = 0.75 * c[1] + 0.25 * c[2];
        out[2] = 0.25 * c[1] + 0.75 * c[2];
        out[3] = 0.75 * c[2] + 0.25 * c[3];
    } else {                                    // co-sited with the even columns: on c1, between c1 and c2, on c2, between c2 and c3
        out[0] = c[1];
        out[1] = 0.5 * c[1] + 0.5 * c[2];
        out[2] = c[2];
        out[3] = 0.5 * c[2] + 0.5 * c[3];
    }
}

// 4 floats to dst[off .. off + n)
__device__ __forceinline__ void store4_f32(float* __restrict__ dst, size_t off, int n, const float (&q)[4]) {
    if (n == 4 && on_grid(dst + off, 16)) {
        *reinterpret_cast<float4*>(dst + off) = make_float4(q[0], q[1], q[2], q[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < n) dst[off + k] = q[k];
    }
}

template <int LAYOUT, bool U8>
__global__ __launch_bounds__(256) void yuv16_to_rgb_kernel(const uint16_t* __restrict__ yp, const uint16_t* __restrict__ up,
                                                           const uint16_t* __restrict__ vp, int H, int W, int quads, ToRgb16 k,
                                                           float* __restrict__ rgb, uint8_t* __restrict__ rgb8) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    const int row = idx / quads, x0 = (idx - row * quads) * 4;
    if (row >= H) return;
    const size_t base = (size_t)row * W + x0, plane = (size_t)H * W;
    const int n = min(4, W - x0);
    double Y[4], U[4], V[4];
    load4_u16(yp, base, n, k.maxc, 0.0, Y);
    if (LAYOUT == VST_YUV_444) {
        load4_u16(up, base, n, k.maxc, k.coff, U);
        load4_u16(vp, base, n, k.maxc, k.coff, V);
    } else {
        const int Hc = LAYOUT == VST_YUV_422 ? H : (H + 1) >> 1, Wc = (W + 1) >> 1;
        chroma4<LAYOUT>(up, Hc, Wc, row, x0, k.maxc, U);
        chroma4<LAYOUT>(vp, Hc, Wc, row, x0, k.maxc, V);
    }
    float r[4], g[4], b[4];
    uint32_t o[12];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const double yy = (Y[p] - k.yoff) * k.iys, pb = (U[p] - k.coff) * k.ics, pr = (V[p] - k.coff) * k.ics;
        const double R = clamp01(yy + k.rv * pr), G = clamp01(yy - k.gv * pr - k.gu * pb), B = clamp01(yy + k.bu * pb);
        r[p] = (float)R, g[p] = (float)G, b[p] = (float)B;
        if (U8) {                               // floor(255 v + 0.5) of the clamped value: 0..255 without a second clamp
            o[3 * p + 0] = (uint32_t)floor(255.0 * R + 0.5);
            o[3 * p + 1] = (uint32_t)floor(255.0 * G + 0.5);
            o[3 * p + 2] = (uint32_t)floor(255.0 * B + 0.5);
        }
    }
    store4_f32(rgb, base, n, r);
    store4_f32(rgb, plane + base, n, g);
    store4_f32(rgb, 2 * plane + base, n, b);
    if (U8) {
        uint8_t* dst = rgb8 + base * 3;
        if (n == 4 && on_grid(dst, 4)) {
            uint32_t* dw = reinterpret_cast<uint32_t*>(dst);
#pragma unroll
            for (int j = 0; j < 3; ++j) dw[j] = o[4 * j] | (o[4 * j + 1] << 8) | (o[4 * j + 2] << 16) | (o[4 * j + 3] << 24);
        } else {
#pragma unroll
            for (int p = 0; p < 4; ++p)
                if (p < n) dst[3 * p] = (uint8_t)o[3 * p], dst[3 * p + 1] = (uint8_t)o[3 * p + 1], dst[3 * p + 2] = (uint8_t)o[3 * p + 2];
        }
    }
}

// 4 pixels of row `row` from column x0 (x0 % 4 == 0, x0 < W), clamped to [0, 1]: columns past the right edge repeat the last one
__device__ __forceinline__ void load_rgb4(const float* __restrict__ rgb, size_t plane, int row, int x0, int W, double (&r)[4],
                                          double (&g)[4], double (&b)[4]) {
    const float* s = rgb + (size_t)row * W + x0;
    if (x0 + 4 <= W && on_grid(s, 16) && on_grid(s + plane, 16) && on_grid(s + 2 * plane, 16)) {
        const float4 fr = *reinterpret_cast<const float4*>(s), fg = *reinterpret_cast<const float4*>(s + plane),
                     fb = *reinterpret_cast<const float4*>(s + 2 * plane);
        r[0] = clamp01(fr.x), r[1] = clamp01(fr.y), r[2] = clamp01(fr.z), r[3] = clamp01(fr.w);
        g[0] = clamp01(fg.x), g[1] = clamp01(fg.y), g[2] = clamp01(fg.z), g[3] = clamp01(fg.w);
        b[0] = clamp01(fb.x), b[1] = clamp01(fb.y), b[2] = clamp01(fb.z), b[3] = clamp01(fb.w);
    } else {
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int d = min(p, W - 1 - x0);
            r[p] = clamp01(s[d]), g[p] = clamp01(s[plane + d]), b[p] = clamp01(s[2 * plane + d]);
        }
    }
}

// 4 codes (already rounded) to dst[off .. off + n): one 8-byte store where the address allows
__device__ __forceinline__ void store4_u16(uint16_t* __restrict__ dst, size_t off, int n, const uint32_t (&q)[4]) {
    if (n == 4 && on_grid(dst + off, 8)) {
        *reinterpret_cast<uint2*>(dst + off) = make_uint2(q[0] | (q[1] << 16), q[2] | (q[3] << 16));
    } else {
#pragma unroll
        for (int p = 0; p < 4; ++p)
            if (p < n) dst[off + p] = (uint16_t)q[p];
    }
}

__global__ __launch_bounds__(256) void rgb_to_yuv16_444_kernel(const float* __restrict__ rgb, int H, int W, int quads, ToYuv16 k,
                                                               uint16_t* __restrict__ yp, uint16_t* __restrict__ up,
                                                               uint16_t* __restrict__ vp) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    const int row = idx / quads, x0 = (idx - row * quads) * 4;
    if (row >= H) return;
    const int n = min(4, W - x0);
    double r[4], g[4], b[4];
    load_rgb4(rgb, (size_t)H * W, row, x0, W, r, g, b);
    uint32_t qy[4], qu[4], qv[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const double Y = k.kr * r[p] + k.kg * g[p] + k.kb * b[p];
        qy[p] = round_code(k.yoff + Y * k.ys, k.maxc);
        qu[p] = round_code(k.coff + (b[p] - Y) * k.icb * k.cs, k.maxc);
        qv[p] = round_code(k.coff + (r[p] - Y) * k.icr * k.cs, k.maxc);
    }
    const size_t base = (size_t)row * W + x0;
    store4_u16(yp, base, n, qy);
    store4_u16(up, base, n, qu);
    store4_u16(vp, base, n, qv);
}

// one lane: luma rows ROWS i .. ROWS i + ROWS - 1 (ROWS = 2 at 4:2:0, 1 at 4:2:2), columns x0 .. x0 + 3 -> 8 bytes of Y per row,
// chroma samples (i, x0 / 2) and (i, x0 / 2 + 1)
template <int LAYOUT>
__global__ __launch_bounds__(256) void rgb_to_yuv16_sub_kernel(const float* __restrict__ rgb, int H, int W, int quads, ToYuv16 k,
                                                               uint16_t* __restrict__ yp, uint16_t* __restrict__ up,
                                                               uint16_t* __restrict__ vp) {
    constexpr int ROWS = LAYOUT == VST_YUV_422 ? 1 : 2;
    constexpr bool PAIRS = LAYOUT == VST_YUV_420_CENTRE;       // columns averaged in pairs; else [1/4, 1/2, 1/4] around the even one
    const int idx = blockIdx.x * 256 + threadIdx.x;
    const int Hc = ROWS == 1 ? H : (H + 1) >> 1, Wc = (W + 1) >> 1;
    const int i = idx / quads, x0 = (idx - i * quads) * 4;
    if (i >= Hc) return;
    const int n = min(4, W - x0);
    const size_t plane = (size_t)H * W;
    double cb[ROWS][5], cr[ROWS][5];            // [row of the lane][column x0 - 1 .. x0 + 3]; column 0 only without PAIRS
#pragma unroll
    for (int dy = 0; dy < ROWS; ++dy) {
        const int row = min(ROWS * i + dy, H - 1);      // odd H: the last row again
        double r[4], g[4], b[4];
        load_rgb4(rgb, plane, row, x0, W, r, g, b);
        uint32_t qy[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const double Y = k.kr * r[p] + k.kg * g[p] + k.kb * b[p];
            qy[p] = round_code(k.yoff + Y * k.ys, k.maxc);
            cb[dy][p + 1] = (b[p] - Y) * k.icb;
            cr[dy][p + 1] = (r[p] - Y) * k.icr;
        }
        if (ROWS * i + dy < H) store4_u16(yp, (size_t)row * W + x0, n, qy);
        if (!PAIRS) {                           // the left neighbour column, re-read from memory (column 0: itself)
            const float* s = rgb + (size_t)row * W + max(x0 - 1, 0);
            const double rr = clamp01(s[0]), gg = clamp01(s[plane]), bb = clamp01(s[2 * plane]);
            const double Y = k.kr * rr + k.kg * gg + k.kb * bb;
            cb[dy][0] = (bb - Y) * k.icb;
            cr[dy][0] = (rr - Y) * k.icr;
        }
    }
    uint32_t qu[2], qv[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {               // chroma column x0 / 2 + j, luma columns x0 + 2 j (- 1), + 1 (load_rgb4 replicated)
        double fb = 0.0, fr = 0.0;
#pragma unroll
        for (int dy = 0; dy < ROWS; ++dy) {
            if (PAIRS) {
                fb += 0.5 * (cb[dy][2 * j + 1] + cb[dy][2 * j + 2]);
                fr += 0.5 * (cr[dy][2 * j + 1] + cr[dy][2 * j + 2]);
            } else {
                fb += 0.25 * cb[dy][2 * j] + 0.5 * cb[dy][2 * j + 1] + 0.25 * cb[dy][2 * j + 2];
                fr += 0.25 * cr[dy][2 * j] + 0.5 * cr[dy][2 * j + 1] + 0.25 * cr[dy][2 * j + 2];
            }
        }
        if (ROWS == 2) fb *= 0.5, fr *= 0.5;
        qu[j] = round_code(k.coff + fb * k.cs, k.maxc);
        qv[j] = round_code(k.coff + fr * k.cs, k.maxc);
    }
    const int jc = x0 >> 1;
    const size_t off = (size_t)i * Wc + jc;
    if (jc + 1 < Wc && on_grid(up + off, 4) && on_grid(vp + off, 4)) {
        *reinterpret_cast<uint32_t*>(up + off) = qu[0] | (qu[1] << 16);
        *reinterpret_cast<uint32_t*>(vp + off) = qv[0] | (qv[1] << 16);
    } else {
        up[off] = (uint16_t)qu[0], vp[off] = (uint16_t)qv[0];
        if (jc + 1 < Wc) up[off + 1] = (uint16_t)qu[1], vp[off + 1] = (uint16_t)qv[1];
    }
}

struct Codes16 {
    double kr, kb, kg, yoff, ys, coff, cs, maxc;
};

bool yuv16_codes(int depth, int matrix, int range, Codes16& c) {
    if (depth < 9 || depth > 16) return false;
    if (matrix == VST_YUV_BT601) c.kr = 0.299, c.kb = 0.114;
    else if (matrix == VST_YUV_BT709) c.kr = 0.2126, c.kb = 0.0722;
    else return false;
    c.kg = 1.0 - c.kr - c.kb;
    const double s = (double)(1 << (depth - 8));
    c.maxc = (double)((1 << depth) - 1);
    c.coff = (double)(1 << (depth - 1));
    if (range == VST_YUV_LIMITED) c.yoff = 16.0 * s, c.ys = 219.0 * s, c.cs = 224.0 * s;
    else if (range == VST_YUV_FULL) c.yoff = 0.0, c.ys = c.maxc, c.cs = c.maxc;
    else return false;
    return true;
}

bool yuv16_args_ok(const void* a, const void* b, const void* c, const void* d, int H, int W, int layout) {
    return a && b && c && d && H >= 1 && W >= 1 && (int64_t)H * W <= VST_MAX_FRAME_PIXELS &&
           (layout == VST_YUV_444 || layout == VST_YUV_420_CENTRE || layout == VST_YUV_420_LEFT || layout == VST_YUV_422);
}

template <int LAYOUT>
void launch_to_rgb(unsigned blocks, hipStream_t st, const uint16_t* y, const uint16_t* u, const uint16_t* v, int H, int W, int quads,
                   const ToRgb16& k, float* rgb, uint8_t* rgb8) {
    if (rgb8) yuv16_to_rgb_kernel<LAYOUT, true><<<blocks, 256, 0, st>>>(y, u, v, H, W, quads, k, rgb, rgb8);
    else yuv16_to_rgb_kernel<LAYOUT, false><<<blocks, 256, 0, st>>>(y, u, v, H, W, quads, k, rgb, rgb8);
}

}  // namespace

extern "C" int vst_yuv16_to_rgb_f32(const uint16_t* y, const uint16_t* u, const uint16_t* v, int H, int W, int depth, int layout,
                                    int matrix, int range, float* rgb_planar, uint8_t* rgb_hwc_u8, void* stream) {
    Codes16 c;
    if (!yuv16_args_ok(y, u, v, rgb_planar, H, W, layout) || !yuv16_codes(depth, matrix, range, c)) return VST_E_ARG;
    ToRgb16 k;
    k.yoff = c.yoff, k.iys = 1.0 / c.ys, k.coff = c.coff, k.ics = 1.0 / c.cs, k.maxc = (uint32_t)c.maxc;
    k.rv = 2.0 * (1.0 - c.kr), k.bu = 2.0 * (1.0 - c.kb);
    k.gv = 2.0 * (1.0 - c.kr) * c.kr / c.kg, k.gu = 2.0 * (1.0 - c.kb) * c.kb / c.kg;
    const int quads = (W + 3) / 4;
    const unsigned blocks = (unsigned)(((int64_t)quads * H + 255) / 256);
    hipStream_t st = (hipStream_t)stream;
    if (layout == VST_YUV_444) launch_to_rgb<VST_YUV_444>(blocks, st, y, u, v, H, W, quads, k, rgb_planar, rgb_hwc_u8);
    else if (layout == VST_YUV_420_CENTRE) launch_to_rgb<VST_YUV_420_CENTRE>(blocks, st, y, u, v, H, W, quads, k, rgb_planar, rgb_hwc_u8);
    else if (layout == VST_YUV_420_LEFT) launch_to_rgb<VST_YUV_420_LEFT>(blocks, st, y, u, v, H, W, quads, k, rgb_planar, rgb_hwc_u8);
    else launch_to_rgb<VST_YUV_422>(blocks, st, y, u, v, H, W, quads, k, rgb_planar, rgb_hwc_u8);
    VST_RETURN_IF_LAUNCH_FAILED();
    return VST_OK;
}

extern "C" int vst_rgb_f32_to_yuv16(const float* rgb_planar, int H, int W, int depth, int layout, int matrix, int range,
                                    uint16_t* y, uint16_t* u, uint16_t* v, void* stream) {
    Codes16 c;
    if (!yuv16_args_ok(y, u, v, rgb_planar, H, W, layout) || !yuv16_codes(depth, matrix, range, c)) return VST_E_ARG;
    ToYuv16 k;
    k.kr = c.kr, k.kg = c.kg, k.kb = c.kb, k.icb = 1.0 / (2.0 * (1.0 - c.kb)), k.icr = 1.0 / (2.0 * (1.0 - c.kr));
    k.yoff = c.yoff, k.ys = c.ys, k.coff = c.coff, k.cs = c.cs, k.maxc = c.maxc;
    const int quads = (W + 3) / 4;
    const int rows = (layout == VST_YUV_444 || layout == VST_YUV_422) ? H : (H + 1) / 2;
    const unsigned blocks = (unsigned)(((int64_t)quads * rows + 255) / 256);
    hipStream_t st = (hipStream_t)stream;
    if (layout == VST_YUV_444) rgb_to_yuv16_444_kernel<<<blocks, 256, 0, st>>>(rgb_planar, H, W, quads, k, y, u, v);
    else if (layout == VST_YUV_420_CENTRE) rgb_to_yuv16_sub_kernel<VST_YUV_420_CENTRE><<<blocks, 256, 0, st>>>(rgb_planar, H, W, quads, k, y, u, v);
    else if (layout == VST_YUV_420_LEFT) rgb_to_yuv16_sub_kernel<VST_YUV_420_LEFT><<<blocks, 256, 0, st>>>(rgb_planar, H, W, quads, k, y, u, v);
    else rgb_to_yuv16_sub_kernel<VST_YUV_422><<<blocks, 256, 0, st>>>(rgb_planar, H, W, quads, k, y, u, v);
    VST_RETURN_IF_LAUNCH_FAILED();
    return VST_OK;
}
