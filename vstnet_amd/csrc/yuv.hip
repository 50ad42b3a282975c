// Raw video edge, both depths (vstnet.h; the arithmetic is stated there and restated in float64 by vstnet_amd/yuv.py):
//   Byte  vst_yuv_to_rgb_u8, vst_rgb_to_yuv_u8: 8-bit Y'CbCr planes <-> the uint8 HWC RGB frame of the video loop, in fp32.
//   Deep  vst_yuv16_to_rgb_f32, vst_rgb_f32_to_yuv16: 9..16-bit planes (little-endian 16-bit samples) <-> fp32 RGB planes
//         [3][H][W] on a 0..1 scale, in fp64 with one rounding at the end (to a code, to a byte of the u8 twin, or to fp32).  At
//         depth 16 a code has magnitude 2^16, where fp32 leaves a quarter of a code of doubt at every rounding; in fp64 the few
//         dozen operations of a pixel err by under 2^-32 of a code, and the operations do not show next to 18 to 30 B per pixel.
// One source: every function below is written once on an edge policy (Byte, Deep) that names the sample, arithmetic and RGB
// types and holds what truly differs - limiting a code to 2^depth - 1 (nothing at 8 bits), the kernels' argument
// structs (chroma offset and top code are literals at 8 bits), the RGB pixel load, the finish.
// Pointwise and launch-latency class.  One lane owns 4 consecutive luma pixels of a row (to RGB, to 4:4:4), a 4 x 2 luma block
// and its two chroma samples (to 4:2:0) or 4 pixels of a row and their two chroma samples (to 4:2:2): 4 samples of Y, 16 bytes
// per fp32 plane and three dwords of u8 RGB per lane where the ADDRESS is on that grid (checked per lane: a pointer needs its
// type's alignment and nothing more, and the planes of one flat Y|U|V buffer start wherever H and W put them), consecutive lanes
// on consecutive addresses; everything else - rows of a width that is no multiple of 4, the ragged right edge, bases off the
// grid - takes guarded narrow accesses.  Chroma neighbours on the way to RGB are read as single samples (a quarter of the
// traffic, and the lanes' columns are adjacent), shared by the lane's 4 pixels.  No LDS, no arrays indexed at run time.
// The one kernel here that is not pointwise is the deep resize's fused first pass (yuv16_resize_h_kernel, below): it converts with
// the same pixel function (rgb4) into LDS and filters from there; resize.hip owns that entry point and the plain passes.
#include <type_traits>

#include "common.h"
#include "deep_resize.h"

namespace {

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }
__device__ __forceinline__ double clamp01(double v) { return fmin(fmax(v, 0.0), 1.0); }
template <class F>
__device__ __forceinline__ uint32_t round_code(F v, F maxc) {  // clamp(floor(v + 0.5), 0, maxc)
    return (uint32_t)fmin(fmax(floor(v + F(0.5)), F(0)), maxc);
}
__device__ __forceinline__ bool on_grid(const void* p, uintptr_t bytes) { return ((uintptr_t)p & (bytes - 1)) == 0; }

// 4 samples in one access: a dword at 8 bits, 8 bytes at 16
__device__ __forceinline__ void read4(const uint8_t* p, uint32_t (&q)[4]) {
    const uint32_t w = *reinterpret_cast<const uint32_t*>(p);
    q[0] = w & 0xffu, q[1] = (w >> 8) & 0xffu, q[2] = (w >> 16) & 0xffu, q[3] = w >> 24;
}
__device__ __forceinline__ void read4(const uint16_t* p, uint32_t (&q)[4]) {
    const uint2 w = *reinterpret_cast<const uint2*>(p);
    q[0] = w.x & 0xffffu, q[1] = w.x >> 16, q[2] = w.y & 0xffffu, q[3] = w.y >> 16;
}
__device__ __forceinline__ void write4(uint8_t* p, const uint32_t (&q)[4]) {
    *reinterpret_cast<uint32_t*>(p) = q[0] | (q[1] << 8) | (q[2] << 16) | (q[3] << 24);
}
__device__ __forceinline__ void write4(uint16_t* p, const uint32_t (&q)[4]) {
    *reinterpret_cast<uint2*>(p) = make_uint2(q[0] | (q[1] << 16), q[2] | (q[3] << 16));
}
__device__ __forceinline__ void write4(float* p, const float (&q)[4]) {
    *reinterpret_cast<float4*>(p) = make_float4(q[0], q[1], q[2], q[3]);
}

// 4 values to dst[off .. off + n): one access where the address allows
template <class T, class Q>
__device__ __forceinline__ void store4(T* __restrict__ dst, size_t off, int n, const Q (&q)[4]) {
    if (n == 4 && on_grid(dst + off, 4 * sizeof(T))) {
        write4(dst + off, q);
    } else {
#pragma unroll
        for (int p = 0; p < 4; ++p)
            if (p < n) dst[off + p] = (T)q[p];
    }
}

// 4 RGB pixels as bytes, o[3 p + channel], to packed HWC: three dwords where the address allows
__device__ __forceinline__ void store_hwc4(uint8_t* __restrict__ dst, int n, const uint32_t (&o)[12]) {
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

struct Byte {           // 8-bit planes, fp32, RGB as packed uint8 HWC on 0..255
    using S = uint8_t;          // a sample
    using S2 = uint16_t;        // two of them
    using F = float;
    using Rgb = uint8_t;
    static constexpr double PEAK = 255.0;       // RGB full scale
    static constexpr bool PLANAR = false, HAS_422 = false;
    static constexpr bool JOINT_READS = true;   // 4:4:4 to RGB: three dword reads one after the other cost 1.3 us at 2160p
    // The kernels' arguments.  The chroma offset and the top code are literals and take no argument bytes: as two more
    // arguments they cost every launch 0.3 to 0.5 us at 1080p, on kernels of 4 to 7 us (profiles/yuv_merge.json).
    struct ToRgb {              // y' = (Y - yoff) ys, pb = (U - coff) cs, pr = (V - coff) cs; R = y' + rv pr ...
        F yoff, ys, cs, rv, gu, gv, bu;
        static constexpr F coff = 128.0f;
        static constexpr uint32_t maxc = 255;
        void depth(double, double) {}
    };
    struct ToYuv {              // Y = kr R + kg G + kb B; Cb = icb (B - Y), Cr = icr (R - Y); codes yoff + ys Y, coff + cs C
        F kr, kg, kb, icb, icr, yoff, ys, cs;
        static constexpr F coff = 128.0f, maxc = 255.0f;
        void depth(double, double) {}
    };
    static __device__ __forceinline__ uint32_t limit(uint32_t c, uint32_t) { return c; }
    static __device__ __forceinline__ F unit(F v) { return v; }
    static __device__ __forceinline__ uint32_t byte(F v) { return round_code(v, 255.0f); }
    static __device__ __forceinline__ uint32_t code(F v, F) { return byte(v); }
    static __device__ __forceinline__ void load_rgb1(const Rgb* __restrict__ rgb, size_t, size_t px, F& r, F& g, F& b) {
        const uint8_t* s = rgb + px * 3;
        r = (F)s[0], g = (F)s[1], b = (F)s[2];
    }
    static __device__ __forceinline__ bool load_rgb4(const Rgb* __restrict__ rgb, size_t, size_t px, F (&r)[4], F (&g)[4], F (&b)[4]) {
        if (!on_grid(rgb + px * 3, 4)) return false;
        const uint32_t* sw = reinterpret_cast<const uint32_t*>(rgb + px * 3);
        const uint32_t w0 = sw[0], w1 = sw[1], w2 = sw[2];
        r[0] = (F)(w0 & 0xffu), g[0] = (F)((w0 >> 8) & 0xffu), b[0] = (F)((w0 >> 16) & 0xffu);
        r[1] = (F)(w0 >> 24), g[1] = (F)(w1 & 0xffu), b[1] = (F)((w1 >> 8) & 0xffu);
        r[2] = (F)((w1 >> 16) & 0xffu), g[2] = (F)(w1 >> 24), b[2] = (F)(w2 & 0xffu);
        r[3] = (F)((w2 >> 8) & 0xffu), g[3] = (F)((w2 >> 16) & 0xffu), b[3] = (F)(w2 >> 24);
        return true;
    }
};

struct Deep {           // 9..16-bit planes, fp64, RGB as fp32 planes [3][H][W] on 0..1 (clamped on the way in and out)
    using S = uint16_t;
    using S2 = uint32_t;
    using F = double;
    using Rgb = float;
    static constexpr double PEAK = 1.0;
    static constexpr bool PLANAR = true, HAS_422 = true;
    static constexpr bool JOINT_READS = false;  // (8-byte reads: the joint form is 0.2 us slower with the u8 twin at 1080p)
    struct ToRgb {              // as Byte::ToRgb, a code first limited to maxc; coff = 2^(depth - 1), maxc = 2^depth - 1
        F yoff, ys, coff, cs, rv, gu, gv, bu;
        uint32_t maxc;
        void depth(double c, double m) { coff = c, maxc = (uint32_t)m; }
    };
    struct ToYuv {
        F kr, kg, kb, icb, icr, yoff, ys, coff, cs, maxc;
        void depth(double c, double m) { coff = c, maxc = m; }
    };
    static __device__ __forceinline__ uint32_t limit(uint32_t c, uint32_t maxc) { return min(c, maxc); }
    static __device__ __forceinline__ F unit(F v) { return clamp01(v); }
    static __device__ __forceinline__ uint32_t byte(F v) { return (uint32_t)floor(255.0 * v + 0.5); }   // v in [0, 1]: no clamp
    static __device__ __forceinline__ uint32_t code(F v, F maxc) { return round_code(v, maxc); }
    static __device__ __forceinline__ void load_rgb1(const Rgb* __restrict__ rgb, size_t plane, size_t px, F& r, F& g, F& b) {
        r = clamp01(rgb[px]), g = clamp01(rgb[plane + px]), b = clamp01(rgb[2 * plane + px]);
    }
    static __device__ __forceinline__ bool load_rgb4(const Rgb* __restrict__ rgb, size_t plane, size_t px, F (&r)[4], F (&g)[4],
                                                     F (&b)[4]) {
        const float* s = rgb + px;
        if (!(on_grid(s, 16) && on_grid(s + plane, 16) && on_grid(s + 2 * plane, 16))) return false;
        const float4 fr = *reinterpret_cast<const float4*>(s), fg = *reinterpret_cast<const float4*>(s + plane),
                     fb = *reinterpret_cast<const float4*>(s + 2 * plane);
        r[0] = clamp01(fr.x), r[1] = clamp01(fr.y), r[2] = clamp01(fr.z), r[3] = clamp01(fr.w);
        g[0] = clamp01(fg.x), g[1] = clamp01(fg.y), g[2] = clamp01(fg.z), g[3] = clamp01(fg.w);
        b[0] = clamp01(fb.x), b[1] = clamp01(fb.y), b[2] = clamp01(fb.z), b[3] = clamp01(fb.w);
        return true;
    }
};

// 4 samples of p[off .. off + n), limited to maxc; `fill` stands in past the edge
template <class E>
__device__ __forceinline__ void load4(const typename E::S* __restrict__ p, size_t off, int n, uint32_t maxc, typename E::F fill,
                                      typename E::F (&out)[4]) {
    using F = typename E::F;
    if (n == 4 && on_grid(p + off, 4 * sizeof(typename E::S))) {
        uint32_t q[4];
        read4(p + off, q);
#pragma unroll
        for (int k = 0; k < 4; ++k) out[k] = (F)E::limit(q[k], maxc);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) out[k] = k < n ? (F)E::limit(p[off + k], maxc) : fill;
    }
}

// 4:4:4, where the edge asks for it (JOINT_READS): the three planes at one offset under ONE check, so that the three reads are
// issued together and waited for once (a check per plane puts each read behind its own branch, one round trip after the other)
template <class E>
__device__ __forceinline__ void load4x3(const typename E::S* __restrict__ yp, const typename E::S* __restrict__ up,
                                        const typename E::S* __restrict__ vp, size_t off, int n, uint32_t maxc, typename E::F coff,
                                        typename E::F (&Y)[4], typename E::F (&U)[4], typename E::F (&V)[4]) {
    using F = typename E::F;
    constexpr uintptr_t GRID = 4 * sizeof(typename E::S);
    if (n == 4 && on_grid(yp + off, GRID) && on_grid(up + off, GRID) && on_grid(vp + off, GRID)) {
        uint32_t qy[4], qu[4], qv[4];
        read4(yp + off, qy), read4(up + off, qu), read4(vp + off, qv);
#pragma unroll
        for (int k = 0; k < 4; ++k) Y[k] = (F)E::limit(qy[k], maxc), U[k] = (F)E::limit(qu[k], maxc), V[k] = (F)E::limit(qv[k], maxc);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            Y[k] = k < n ? (F)E::limit(yp[off + k], maxc) : F(0);
            U[k] = k < n ? (F)E::limit(up[off + k], maxc) : coff;
            V[k] = k < n ? (F)E::limit(vp[off + k], maxc) : coff;
        }
    }
}

// Chroma of the 4 luma pixels (yl, x0 .. x0 + 3), x0 % 4 == 0, from a subsampled plane of Hc x Wc samples.  The chroma coordinate
// of luma x is (x - 1/2) / 2 (centre) or x / 2 (left, 4:2:2), so the pixels read the columns x0 / 2 - 1 .. x0 / 2 + 2; of luma y
// (y - 1/2) / 2 at 4:2:0 - two rows, blended first - and y itself at 4:2:2.  Indices are clamped to the plane (a lane at the
// ragged right edge reads clamped columns for the pixels it does not store).  Exact: the weights are multiples of 1/4 and the
// values integers, so the order of the two blends changes nothing.
template <int LAYOUT, class E>
__device__ __forceinline__ void chroma4(const typename E::S* __restrict__ p, int Hc, int Wc, int yl, int x0, uint32_t maxc,
                                        typename E::F (&out)[4]) {
    using F = typename E::F;
    // even rows sit 3/4 of the way from sample yl / 2 - 1 to yl / 2, odd rows 1/4 of the way from yl / 2 to yl / 2 + 1
    const int i0 = (yl >> 1) - ((yl & 1) ? 0 : 1);
    const F wy = (yl & 1) ? F(0.25) : F(0.75);
    const typename E::S* ra = p + (size_t)(LAYOUT == VST_YUV_422 ? yl : clampi(i0, Hc - 1)) * Wc;
    const typename E::S* rb = p + (size_t)clampi(i0 + 1, Hc - 1) * Wc;
    const int j0 = (x0 >> 1) - 1;
    F c[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int j = clampi(j0 + k, Wc - 1);
        c[k] = (F)E::limit(ra[j], maxc);
        if (LAYOUT != VST_YUV_422) c[k] = (F(1) - wy) * c[k] + wy * (F)E::limit(rb[j], maxc);
    }
    if (LAYOUT == VST_YUV_420_CENTRE) {         // x0: 3/4 from c0 to c1; x0 + 1, + 2: 1/4 and 3/4 from c1 to c2; x0 + 3: 1/4 from c2 to c3
        out[0] = F(0.25) * c[0] + F(0.75) * c[1];
        out[1] = F(0.75) * c[1] + F(0.25) * c[2];
        out[2] = F(0.25) * c[1] + F(0.75) * c[2];
        out[3] = F(0.75) * c[2] + F(0.25) * c[3];
    } else {                                    // co-sited with the even columns: on c1, between c1 and c2, on c2, between c2 and c3
        out[0] = c[1];
        out[1] = F(0.5) * c[1] + F(0.5) * c[2];
        out[2] = c[2];
        out[3] = F(0.5) * c[2] + F(0.5) * c[3];
    }
}

// The pixel arithmetic of the way to RGB, shared by every kernel that converts: R, G, B of the 4 luma pixels (row, x0 .. x0 + 3),
// x0 % 4 == 0 and x0 < W, of which n = min(4, W - x0) exist - the codes limited, chroma at the luma positions, the matrix, the
// edge's clamp.
template <int LAYOUT, class E>
__device__ __forceinline__ void rgb4(const typename E::S* __restrict__ yp, const typename E::S* __restrict__ up,
                                     const typename E::S* __restrict__ vp, int H, int W, int row, int x0, int n,
                                     const typename E::ToRgb& k, typename E::F (&R)[4], typename E::F (&G)[4],
                                     typename E::F (&B)[4]) {
    using F = typename E::F;
    const size_t base = (size_t)row * W + x0;
    F Y[4], U[4], V[4];
    if (LAYOUT == VST_YUV_444 && E::JOINT_READS) {
        load4x3<E>(yp, up, vp, base, n, k.maxc, k.coff, Y, U, V);
    } else {
        load4<E>(yp, base, n, k.maxc, F(0), Y);
        if (LAYOUT == VST_YUV_444) {
            load4<E>(up, base, n, k.maxc, k.coff, U);
            load4<E>(vp, base, n, k.maxc, k.coff, V);
        } else {
            const int Hc = LAYOUT == VST_YUV_422 ? H : (H + 1) >> 1, Wc = (W + 1) >> 1;
            chroma4<LAYOUT, E>(up, Hc, Wc, row, x0, k.maxc, U);
            chroma4<LAYOUT, E>(vp, Hc, Wc, row, x0, k.maxc, V);
        }
    }
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const F yy = (Y[p] - k.yoff) * k.ys, pb = (U[p] - k.coff) * k.cs, pr = (V[p] - k.coff) * k.cs;
        R[p] = E::unit(yy + k.rv * pr), G[p] = E::unit(yy - k.gv * pr - k.gu * pb), B[p] = E::unit(yy + k.bu * pb);
    }
}

// rgbf: the Deep edge's fp32 planes; rgb8: packed uint8 HWC, written if U8 (the Byte edge's output, the Deep edge's optional twin)
template <int LAYOUT, class E, bool U8>
__global__ __launch_bounds__(256) void yuv_to_rgb_kernel(const typename E::S* __restrict__ yp, const typename E::S* __restrict__ up,
                                                         const typename E::S* __restrict__ vp, int H, int W, int quads,
                                                         typename E::ToRgb k, float* __restrict__ rgbf,
                                                         uint8_t* __restrict__ rgb8) {
    using F = typename E::F;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    const int row = idx / quads, x0 = (idx - row * quads) * 4;
    if (row >= H) return;
    const size_t base = (size_t)row * W + x0, plane = (size_t)H * W;
    const int n = min(4, W - x0);
    F R[4], G[4], B[4];
    rgb4<LAYOUT, E>(yp, up, vp, H, W, row, x0, n, k, R, G, B);
    float r[4], g[4], b[4];
    uint32_t o[12];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        r[p] = (float)R[p], g[p] = (float)G[p], b[p] = (float)B[p];    // (what the PLANAR stores take: dead code at 8 bits)
        if (U8) o[3 * p + 0] = E::byte(R[p]), o[3 * p + 1] = E::byte(G[p]), o[3 * p + 2] = E::byte(B[p]);
    }
    if (E::PLANAR) {
        store4(rgbf, base, n, r);
        store4(rgbf, plane + base, n, g);
        store4(rgbf, 2 * plane + base, n, b);
    }
    if (U8) store_hwc4(rgb8 + base * 3, n, o);
}

// The deep resize's first pass where that is horizontal (vst_yuv16_img_resize_f32, resize.hip; DESIGN.md section 6, "Deep
// resize"): 16-bit planes at the source size -> fp32 planes [3][H][Wd], with no source-size RGB frame in memory.  A workgroup owns
// DEEP_H_PIX output columns of `rows_per` consecutive rows.  It converts the source span of its columns once - rgb4 above, a quad
// per lane and turn, rounded to fp32 as vst_yuv16_to_rgb_f32 stores it - into LDS, lds[row][channel][span_cap], and filters from
// there: a lane owns one (row, column) and its three channels, Pillow's double weights from the table (L1/L2: a column's row of
// weights is contiguous), fp64 accumulation, one rounding to fp32.  FINAL: this pass is the frame's last, so the value is clamped
// to [0, 1] and goes to the output planes and, if asked for, the u8 twin (vst_deep_final_store).
template <int LAYOUT, bool FINAL>
__global__ __launch_bounds__(256) void yuv16_resize_h_kernel(const uint16_t* __restrict__ yp, const uint16_t* __restrict__ up,
                                                             const uint16_t* __restrict__ vp, int H, int W, Deep::ToRgb k,
                                                             const int* __restrict__ table, int Wd, int ksize, int col_tiles,
                                                             int rows_per, int span_cap, float* __restrict__ dst,
                                                             uint8_t* __restrict__ dst_u8) {
    extern __shared__ float span_lds[];         // [rows_per][3][span_cap]
    const int ct = blockIdx.x % col_tiles;
    const int y0 = (blockIdx.x / col_tiles) * rows_per;
    const int x0 = ct * DEEP_H_PIX;
    const int npix = min(DEEP_H_PIX, Wd - x0);
    const int nr = min(rows_per, H - y0);
    const int tid = threadIdx.x;
    const double* __restrict__ coef = reinterpret_cast<const double*>(table + 2 * (size_t)Wd);
    // the span: from the first column's first tap (down to the quad grid) to the last column's last tap; both ends grow with the
    // column, so every column's taps lie inside.  (span_cap is the host's bound on it; the min only states that.)
    const int s0 = table[2 * (size_t)x0] & ~3;
    const int last = x0 + npix - 1;
    const int span = min(min(table[2 * (size_t)last] + table[2 * (size_t)last + 1], W) - s0, span_cap);
    const int quads = (span + 3) >> 2;
    for (int i = tid; i < nr * quads; i += 256) {
        const int r = i / quads, q = i - r * quads;
        const int xs = s0 + 4 * q;
        double R[4], G[4], B[4];
        rgb4<LAYOUT, Deep>(yp, up, vp, H, W, y0 + r, xs, min(4, W - xs), k, R, G, B);
        float* l = span_lds + (size_t)r * 3 * span_cap + 4 * q;
#pragma unroll
        for (int p = 0; p < 4; ++p) l[p] = (float)R[p], l[span_cap + p] = (float)G[p], l[2 * span_cap + p] = (float)B[p];
    }
    __syncthreads();
    const size_t plane = (size_t)H * Wd;
    for (int o = tid; o < nr * npix; o += 256) {
        const int r = o / npix, x = x0 + (o - r * npix);
        const int first = table[2 * (size_t)x], n = table[2 * (size_t)x + 1];
        const double* __restrict__ kk = coef + (size_t)x * ksize;
        const float* l = span_lds + (size_t)r * 3 * span_cap + (first - s0);
        double a0 = 0.0, a1 = 0.0, a2 = 0.0;
        for (int j = 0; j < n; ++j) {
            const double c = kk[j];
            a0 = fma((double)l[j], c, a0), a1 = fma((double)l[span_cap + j], c, a1), a2 = fma((double)l[2 * span_cap + j], c, a2);
        }
        const int y = y0 + r;
        if (FINAL) {
            vst_deep_final_store(dst, dst_u8, plane, Wd, 0, y, x, a0);
            vst_deep_final_store(dst, dst_u8, plane, Wd, 1, y, x, a1);
            vst_deep_final_store(dst, dst_u8, plane, Wd, 2, y, x, a2);
        } else {
            const size_t px = (size_t)y * Wd + x;
            dst[px] = (float)a0, dst[plane + px] = (float)a1, dst[2 * plane + px] = (float)a2;
        }
    }
}

// 4 pixels of row `row` from column x0 (x0 % 4 == 0, x0 < W): columns past the right edge repeat the last one
template <class E>
__device__ __forceinline__ void load_rgb4(const typename E::Rgb* __restrict__ rgb, size_t plane, int row, int x0, int W,
                                          typename E::F (&r)[4], typename E::F (&g)[4], typename E::F (&b)[4]) {
    if (x0 + 4 <= W && E::load_rgb4(rgb, plane, (size_t)row * W + x0, r, g, b)) return;
#pragma unroll
    for (int p = 0; p < 4; ++p) E::load_rgb1(rgb, plane, (size_t)row * W + min(x0 + p, W - 1), r[p], g[p], b[p]);
}

// one lane: luma rows ROWS i .. ROWS i + ROWS - 1 (ROWS = 2 at 4:2:0, else 1), columns x0 .. x0 + 3 -> 4 samples of Y per row
// and the chroma samples of those pixels: 4 at 4:4:4, else (i, x0 / 2) and (i, x0 / 2 + 1)
template <int LAYOUT, class E>
__global__ __launch_bounds__(256) void rgb_to_yuv_kernel(const typename E::Rgb* __restrict__ rgb, int H, int W, int quads,
                                                         typename E::ToYuv k, typename E::S* __restrict__ yp,
                                                         typename E::S* __restrict__ up, typename E::S* __restrict__ vp) {
    using F = typename E::F;
    using S2 = typename E::S2;
    constexpr int ROWS = (LAYOUT == VST_YUV_420_CENTRE || LAYOUT == VST_YUV_420_LEFT) ? 2 : 1;
    constexpr bool SUB = LAYOUT != VST_YUV_444;
    constexpr bool PAIRS = LAYOUT == VST_YUV_420_CENTRE;       // columns averaged in pairs; else [1/4, 1/2, 1/4] around the even one
    const int idx = blockIdx.x * 256 + threadIdx.x;
    const int Hc = ROWS == 1 ? H : (H + 1) >> 1, Wc = (W + 1) >> 1;
    const int i = idx / quads, x0 = (idx - i * quads) * 4;
    if (i >= Hc) return;
    const int n = min(4, W - x0);
    const size_t plane = (size_t)H * W;
    F cb[ROWS][5], cr[ROWS][5];                 // [row of the lane][column x0 - 1 .. x0 + 3]; column 0 only for the 3-tap filter
#pragma unroll
    for (int dy = 0; dy < ROWS; ++dy) {
        const int row = min(ROWS * i + dy, H - 1);      // odd H: the last row again
        F r[4], g[4], b[4];
        load_rgb4<E>(rgb, plane, row, x0, W, r, g, b);
        uint32_t qy[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const F Y = k.kr * r[p] + k.kg * g[p] + k.kb * b[p];
            qy[p] = E::code(k.yoff + Y * k.ys, k.maxc);
            cb[dy][p + 1] = (b[p] - Y) * k.icb;
            cr[dy][p + 1] = (r[p] - Y) * k.icr;
        }
        if (ROWS * i + dy < H) store4(yp, (size_t)row * W + x0, n, qy);
        if (SUB && !PAIRS) {                    // the left neighbour column, re-read from memory (column 0: itself)
            F rr, gg, bb;
            E::load_rgb1(rgb, plane, (size_t)row * W + max(x0 - 1, 0), rr, gg, bb);
            const F Y = k.kr * rr + k.kg * gg + k.kb * bb;
            cb[dy][0] = (bb - Y) * k.icb;
            cr[dy][0] = (rr - Y) * k.icr;
        }
    }
    if (!SUB) {
        uint32_t qu[4], qv[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            qu[p] = E::code(k.coff + cb[0][p + 1] * k.cs, k.maxc);
            qv[p] = E::code(k.coff + cr[0][p + 1] * k.cs, k.maxc);
        }
        store4(up, (size_t)i * W + x0, n, qu);
        store4(vp, (size_t)i * W + x0, n, qv);
        return;
    }
    uint32_t qu[2], qv[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {               // chroma column x0 / 2 + j, luma columns x0 + 2 j (- 1), + 1 (load_rgb4 replicated)
        F fb = 0, fr = 0;
#pragma unroll
        for (int dy = 0; dy < ROWS; ++dy) {
            if (PAIRS) {                        // the sum of the 2 x 2 block, scaled below: every scaling is by a power of two
                fb += cb[dy][2 * j + 1] + cb[dy][2 * j + 2];
                fr += cr[dy][2 * j + 1] + cr[dy][2 * j + 2];
            } else {
                fb += F(0.25) * cb[dy][2 * j] + F(0.5) * cb[dy][2 * j + 1] + F(0.25) * cb[dy][2 * j + 2];
                fr += F(0.25) * cr[dy][2 * j] + F(0.5) * cr[dy][2 * j + 1] + F(0.25) * cr[dy][2 * j + 2];
            }
        }
        if (ROWS == 2) fb *= F(PAIRS ? 0.25 : 0.5), fr *= F(PAIRS ? 0.25 : 0.5);
        qu[j] = E::code(k.coff + fb * k.cs, k.maxc);
        qv[j] = E::code(k.coff + fr * k.cs, k.maxc);
    }
    const int jc = x0 >> 1;
    const size_t off = (size_t)i * Wc + jc;
    if (jc + 1 < Wc && on_grid(up + off, sizeof(S2)) && on_grid(vp + off, sizeof(S2))) {
        *reinterpret_cast<S2*>(up + off) = (S2)(qu[0] | (qu[1] << (8 * sizeof(typename E::S))));
        *reinterpret_cast<S2*>(vp + off) = (S2)(qv[0] | (qv[1] << (8 * sizeof(typename E::S))));
    } else {
        up[off] = (typename E::S)qu[0], vp[off] = (typename E::S)qv[0];
        if (jc + 1 < Wc) up[off + 1] = (typename E::S)qu[1], vp[off + 1] = (typename E::S)qv[1];
    }
}

// What (matrix, range, depth) mean, in double: depth 8 is the Byte edge.  s = 2^(depth - 8) scales the limited range.
struct Codes {
    double kr, kb, kg, yoff, ys, coff, cs, maxc;
};

bool yuv_codes(int depth, int matrix, int range, Codes& c) {
    if (depth < 8 || depth > 16) return false;
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

bool args_ok(const void* a, const void* b, const void* c, const void* d, int H, int W, int layout, bool with_422) {
    return a && b && c && d && H >= 1 && W >= 1 && (int64_t)H * W <= VST_MAX_FRAME_PIXELS &&
           (layout == VST_YUV_444 || layout == VST_YUV_420_CENTRE || layout == VST_YUV_420_LEFT ||
            (with_422 && layout == VST_YUV_422));
}

// fn(layout as a compile-time constant), for the layouts the edge has
template <class E, class Fn>
void with_layout(int layout, Fn fn) {
    if (layout == VST_YUV_444) fn(std::integral_constant<int, VST_YUV_444>());
    else if (layout == VST_YUV_420_CENTRE) fn(std::integral_constant<int, VST_YUV_420_CENTRE>());
    else if (layout == VST_YUV_420_LEFT) fn(std::integral_constant<int, VST_YUV_420_LEFT>());
    else if constexpr (E::HAS_422) fn(std::integral_constant<int, VST_YUV_422>());
}

// the kernels' constants of the way to RGB
template <class E>
typename E::ToRgb to_rgb_args(const Codes& c) {
    using F = typename E::F;
    typename E::ToRgb k;
    k.depth(c.coff, c.maxc);
    k.yoff = (F)c.yoff, k.ys = (F)(E::PEAK / c.ys), k.cs = (F)(E::PEAK / c.cs);
    k.rv = (F)(2.0 * (1.0 - c.kr)), k.bu = (F)(2.0 * (1.0 - c.kb));
    k.gv = (F)(2.0 * (1.0 - c.kr) * c.kr / c.kg), k.gu = (F)(2.0 * (1.0 - c.kb) * c.kb / c.kg);
    return k;
}

template <class E, bool U8>
int yuv_to_rgb(const typename E::S* y, const typename E::S* u, const typename E::S* v, int H, int W, int depth, int layout,
               int matrix, int range, float* rgbf, uint8_t* rgb8, void* stream) {
    Codes c;
    if (!args_ok(y, u, v, E::PLANAR ? (const void*)rgbf : rgb8, H, W, layout, E::HAS_422) || !yuv_codes(depth, matrix, range, c))
        return VST_E_ARG;
    const typename E::ToRgb k = to_rgb_args<E>(c);
    const int quads = (W + 3) / 4;
    const unsigned blocks = (unsigned)(((int64_t)quads * H + 255) / 256);
    with_layout<E>(layout, [&](auto L) {
        yuv_to_rgb_kernel<decltype(L)::value, E, U8><<<blocks, 256, 0, (hipStream_t)stream>>>(y, u, v, H, W, quads, k, rgbf, rgb8);
    });
    VST_RETURN_IF_LAUNCH_FAILED();
    return VST_OK;
}

template <class E>
int rgb_to_yuv(const typename E::Rgb* rgb, int H, int W, int depth, int layout, int matrix, int range, typename E::S* y,
               typename E::S* u, typename E::S* v, void* stream) {
    using F = typename E::F;
    Codes c;
    if (!args_ok(y, u, v, rgb, H, W, layout, E::HAS_422) || !yuv_codes(depth, matrix, range, c)) return VST_E_ARG;
    typename E::ToYuv k;
    k.depth(c.coff, c.maxc);
    k.kr = (F)c.kr, k.kb = (F)c.kb, k.kg = (F)c.kg;
    k.icb = (F)(1.0 / (2.0 * (1.0 - c.kb))), k.icr = (F)(1.0 / (2.0 * (1.0 - c.kr)));
    k.yoff = (F)c.yoff, k.ys = (F)(c.ys / E::PEAK), k.cs = (F)(c.cs / E::PEAK);
    const int quads = (W + 3) / 4;
    const int rows = (layout == VST_YUV_444 || layout == VST_YUV_422) ? H : (H + 1) / 2;
    const unsigned blocks = (unsigned)(((int64_t)quads * rows + 255) / 256);
    with_layout<E>(layout, [&](auto L) {
        rgb_to_yuv_kernel<decltype(L)::value, E><<<blocks, 256, 0, (hipStream_t)stream>>>(rgb, H, W, quads, k, y, u, v);
    });
    VST_RETURN_IF_LAUNCH_FAILED();
    return VST_OK;
}

}  // namespace

extern "C" int vst_yuv_to_rgb_u8(const uint8_t* y, const uint8_t* u, const uint8_t* v, int H, int W, int layout, int matrix,
                                 int range, uint8_t* rgb_hwc, void* stream) {
    return yuv_to_rgb<Byte, true>(y, u, v, H, W, 8, layout, matrix, range, nullptr, rgb_hwc, stream);
}

extern "C" int vst_rgb_to_yuv_u8(const uint8_t* rgb_hwc, int H, int W, int layout, int matrix, int range, uint8_t* y,
                                 uint8_t* u, uint8_t* v, void* stream) {
    return rgb_to_yuv<Byte>(rgb_hwc, H, W, 8, layout, matrix, range, y, u, v, stream);
}

extern "C" int vst_yuv16_to_rgb_f32(const uint16_t* y, const uint16_t* u, const uint16_t* v, int H, int W, int depth, int layout,
                                    int matrix, int range, float* rgb_planar, uint8_t* rgb_hwc_u8, void* stream) {
    if (depth < 9) return VST_E_ARG;
    return rgb_hwc_u8 ? yuv_to_rgb<Deep, true>(y, u, v, H, W, depth, layout, matrix, range, rgb_planar, rgb_hwc_u8, stream)
                      : yuv_to_rgb<Deep, false>(y, u, v, H, W, depth, layout, matrix, range, rgb_planar, rgb_hwc_u8, stream);
}

extern "C" int vst_rgb_f32_to_yuv16(const float* rgb_planar, int H, int W, int depth, int layout, int matrix, int range,
                                    uint16_t* y, uint16_t* u, uint16_t* v, void* stream) {
    if (depth < 9) return VST_E_ARG;
    return rgb_to_yuv<Deep>(rgb_planar, H, W, depth, layout, matrix, range, y, u, v, stream);
}

// resize.hip's side of the deep resize (deep_resize.h)
int vst_deep_yuv_check(const void* y, const void* u, const void* v, int H, int W, int depth, int layout, int matrix, int range) {
    Codes c;
    const bool ok = depth >= 9 && args_ok(y, u, v, y, H, W, layout, true) && yuv_codes(depth, matrix, range, c);
    return ok ? VST_OK : VST_E_ARG;
}

int vst_deep_resize_h_fused(const uint16_t* y, const uint16_t* u, const uint16_t* v, int H, int W, int depth, int layout,
                            int matrix, int range, const int* table, int Wd, int ksize, float* dst, uint8_t* dst_u8, int final,
                            hipStream_t st) {
    Codes c;
    if (depth < 9 || !args_ok(y, u, v, dst, H, W, layout, true) || !yuv_codes(depth, matrix, range, c) || !table || Wd < 1 ||
        Wd > W || (final ? false : dst_u8 != nullptr))
        return VST_E_ARG;
    const Deep::ToRgb k = to_rgb_args<Deep>(c);
    // the span of DEEP_H_PIX columns: (PIX - 1) * scale between the first and the last centre, the support on either side (ksize
    // >= 2 * support + 1), the rounding of the two ends and the quad grid
    const int span_cap = ((int)(((int64_t)DEEP_H_PIX * W + Wd - 1) / Wd) + ksize + 4 + 3) & ~3;
    const size_t row_bytes = (size_t)3 * span_cap * sizeof(float);
    int rows_per = (int)(DEEP_H_LDS_BYTES / row_bytes);
    rows_per = rows_per < 1 ? 1 : (rows_per > 8 ? 8 : rows_per);
    const int col_tiles = (Wd + DEEP_H_PIX - 1) / DEEP_H_PIX;
    const int64_t blocks = (int64_t)col_tiles * ((H + rows_per - 1) / rows_per);
    if (blocks > 0x7fffffffLL || rows_per * row_bytes > 64 * 1024) return VST_E_SHAPE;
    with_layout<Deep>(layout, [&](auto L) {
        constexpr int LAY = decltype(L)::value;
        if (final)
            yuv16_resize_h_kernel<LAY, true><<<(unsigned)blocks, 256, rows_per * row_bytes, st>>>(
                y, u, v, H, W, k, table, Wd, ksize, col_tiles, rows_per, span_cap, dst, dst_u8);
        else
            yuv16_resize_h_kernel<LAY, false><<<(unsigned)blocks, 256, rows_per * row_bytes, st>>>(
                y, u, v, H, W, k, table, Wd, ksize, col_tiles, rows_per, span_cap, dst, dst_u8);
    });
    VST_RETURN_IF_LAUNCH_FAILED();
    return VST_OK;
}
