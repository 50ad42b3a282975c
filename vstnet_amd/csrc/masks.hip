// Mask producers (vstnet.h, "mask producers"): everything a per-frame label map needs before the masked transfer, on the
// device and in stream order - colours to labels (utils/utils.py:104-137 of the reference), histograms, the remapping of
// models/segmentation/SegReMapping.py:19-76 as a 256-entry table, the label plan from histograms, and the one fused pass
// over an uploaded map (colours -> labels -> histogram -> labels in the packed code's row order).
#include "common.h"

namespace {

// the reference's colour dictionary in its order (utils/utils.py:106-116): first minimum of the L1 distance wins
__device__ __forceinline__ unsigned color_label(int r, int g, int b) {
    constexpr int K = 9;
    constexpr int cr[K] = {0, 0, 0, 255, 255, 255, 128, 0, 255};
    constexpr int cg[K] = {0, 255, 0, 255, 0, 255, 128, 255, 0};
    constexpr int cb[K] = {255, 0, 0, 255, 0, 0, 128, 255, 255};
    constexpr unsigned lab[K] = {3, 2, 0, 1, 4, 5, 6, 7, 8};
    int best = 1 << 20;
    unsigned out = 0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int d = abs(r - cr[k]) + abs(g - cg[k]) + abs(b - cb[k]);
        if (d < best) { best = d; out = lab[k]; }
    }
    return out;
}

// labels of 4 consecutive pixels, one per byte (pixel 0 in the low byte).  p is 4-byte aligned (W % 4 == 0).
template <bool COLOURS>
__device__ __forceinline__ unsigned load4(const uint8_t* __restrict__ src, size_t pixel) {
    if (!COLOURS) return *(const unsigned*)(src + pixel);
    const unsigned* q = (const unsigned*)(src + pixel * 3);
    const unsigned a = q[0], b = q[1], c = q[2];          // r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3
    return color_label(a & 255, (a >> 8) & 255, (a >> 16) & 255) |
           color_label(a >> 24, b & 255, (b >> 8) & 255) << 8 |
           color_label((b >> 16) & 255, b >> 24, c & 255) << 16 |
           color_label((c >> 8) & 255, (c >> 16) & 255, c >> 24) << 24;
}

__global__ __launch_bounds__(256) void colors_to_labels_kernel(const uint8_t* __restrict__ rgb, uint8_t* __restrict__ out, long n) {
    for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < n; p += (long)gridDim.x * 256)
        out[p] = (uint8_t)color_label(rgb[3 * p], rgb[3 * p + 1], rgb[3 * p + 2]);
}

__global__ __launch_bounds__(256) void hist_kernel(const uint8_t* __restrict__ mask, long L, int* __restrict__ hist) {
    __shared__ int h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < L; p += (long)gridDim.x * 256) atomicAdd(&h[mask[p]], 1);
    __syncthreads();
    if (h[threadIdx.x]) atomicAdd(&hist[threadIdx.x], h[threadIdx.x]);
}

__global__ __launch_bounds__(256) void apply_lut_kernel(const uint8_t* in, const uint8_t* __restrict__ lut, uint8_t* out, long n) {
    __shared__ uint8_t t[256];
    t[threadIdx.x] = lut[threadIdx.x];
    __syncthreads();
    for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < n; p += (long)gridDim.x * 256) out[p] = t[in[p]];
}

// The fused pass.  One thread owns one half (i) of two consecutive 4 x 4 pixel cells: per cell it reads 4 pixels of the image
// rows 4h + 2i and 4h + 2i + 1 (one dword of labels or three of colours each: neighbouring threads read neighbouring
// cells, a wave reads contiguous row segments) and writes the cell's 8 row labels, g = 4j + 2i' + j' <-> pixel
// (4h + 2i + i', 4w + 2j + j') (mask_to_code_kernel's mapping); the two cells' 16 bytes go out as one store where the
// half's base is 16-byte aligned.  Histogram: runs of equal labels are counted in registers first (a label map is made of
// runs), then one LDS atomic per run into the wave's own bins, then one global atomic per non-empty bin and workgroup.
template <bool COLOURS>
__global__ __launch_bounds__(256) void mask_prepare_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ rows,
                                                           int* __restrict__ hist, int Hq, int Wq) {
    __shared__ int h[4][256];
    for (int k = threadIdx.x; k < 4 * 256; k += 256) (&h[0][0])[k] = 0;
    __syncthreads();
    const long cells = (long)Hq * Wq, pairs = (cells + 1) >> 1;
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t < 2 * pairs) {
        const int i = t >= pairs;
        const long c0 = 2 * (t - (long)i * pairs);
        const int W = 4 * Wq;
        unsigned out[4] = {0, 0, 0, 0};
        const int ncell = c0 + 1 < cells ? 2 : 1;
        int* hw = h[threadIdx.x >> 6];
        unsigned run_label = 0;
        int run = 0;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            if (c >= ncell) break;
            const long cell = c0 + c;
            const int hh = (int)(cell / Wq), ww = (int)(cell - (long)hh * Wq);
            const size_t p0 = (size_t)(4 * hh + 2 * i) * W + 4 * ww;
            const unsigned a = load4<COLOURS>(src, p0), b = load4<COLOURS>(src, p0 + W);      // rows i' = 0, 1; x = 0..3 in bytes
            // g0..g3 = (0,x0) (0,x1) (1,x0) (1,x1); g4..g7 = (0,x2) (0,x3) (1,x2) (1,x3)
            out[2 * c] = (a & 0xffffu) | (b << 16);
            out[2 * c + 1] = (a >> 16) | (b & 0xffff0000u);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const unsigned l = (out[2 * c + (k >> 2)] >> (8 * (k & 3))) & 255u;
                if (l == run_label) ++run;
                else {
                    if (run) atomicAdd(&hw[run_label], run);
                    run_label = l; run = 1;
                }
            }
        }
        if (run) atomicAdd(&hw[run_label], run);
        uint8_t* dst = rows + (size_t)i * cells * 8 + (size_t)c0 * 8;
        if (ncell == 2 && (((size_t)dst) & 15) == 0) *(u32x4*)dst = u32x4{out[0], out[1], out[2], out[3]};
        else {
            *(uint2*)dst = make_uint2(out[0], out[1]);
            if (ncell == 2) *(uint2*)(dst + 8) = make_uint2(out[2], out[3]);
        }
    }
    __syncthreads();
    const int v = h[0][threadIdx.x] + h[1][threadIdx.x] + h[2][threadIdx.x] + h[3][threadIdx.x];
    if (v) atomicAdd(&hist[threadIdx.x], v);
}

// One workgroup, thread l = label l.  See vstnet.h for the rules; `related` walks column l of the table.
__global__ __launch_bounds__(256) void remap_lut_kernel(const int* __restrict__ hist, const int* __restrict__ style_hist,
                                                        const int16_t* __restrict__ table, int rows, int cols, int min_count,
                                                        uint8_t* __restrict__ lut, int* __restrict__ hist_out,
                                                        unsigned* __restrict__ flags) {
    __shared__ int h0[256], h1[256], h2[256], sh[256];
    __shared__ unsigned char self_lut[256], cross_lut[256];
    const int l = threadIdx.x;
    h0[l] = hist[l];
    h1[l] = h2[l] = 0;
    sh[l] = style_hist ? style_hist[l] : 1;
    __syncthreads();
    unsigned flag = 0;
    int to = l;
    if (h0[l] > 0 && h0[l] < min_count) {              // self_remapping: shares are those of the ORIGINAL map
        if (l >= cols) flag = VST_MASK_OUT_OF_TABLE;
        else
            for (int j = 0; j < rows; ++j) {
                const int cand = table[(size_t)j * cols + l];
                if (cand >= 0 && cand < 256 && h0[cand] > 0 && h0[cand] >= min_count) { to = cand; break; }
            }
    }
    self_lut[l] = (unsigned char)to;
    if (h0[l] > 0) atomicAdd(&h1[to], h0[l]);
    __syncthreads();
    to = l;
    if (style_hist && h1[l] > 0 && sh[l] <= 0) {        // cross_remapping of the self-remapped map
        if (l >= cols) flag = VST_MASK_OUT_OF_TABLE;
        else
            for (int j = 0; j < rows; ++j) {
                const int cand = table[(size_t)j * cols + l];
                if (cand >= 0 && cand < 256 && sh[cand] > 0) { to = cand; break; }
            }
    }
    cross_lut[l] = (unsigned char)to;
    if (h1[l] > 0) atomicAdd(&h2[to], h1[l]);
    __syncthreads();
    lut[l] = h0[l] > 0 ? cross_lut[self_lut[l]] : (unsigned char)l;
    if (hist_out) hist_out[l] = h2[l];
    if (flag && flags) atomicOr(flags, flag);
}

// the style histograms of a plan against several style maps (vst_label_plan_hists); one entry for vst_label_plan_hist
struct StyleHists {
    const int* h[CWCT_MAX_STYLES];
    int n;
};

__global__ __launch_bounds__(256) void label_plan_hist_kernel(const int* __restrict__ hist_c, const uint8_t* __restrict__ remap,
                                                              const StyleHists hs, int cap, LabelPlan* plan, unsigned* flags) {
    __shared__ int hc[256], valid[256];
    __shared__ unsigned char slot_of[256];
    const int l = threadIdx.x;
    hc[l] = 0;
    __syncthreads();
    const int to = remap ? remap[l] : l;
    const int raw = hist_c[l];
    if (raw > 0) atomicAdd(&hc[to], raw);
    __syncthreads();
    const int a = hc[l];
    // the validity rule exactly as label_plan_kernel states it (cWCT.py:178), against EVERY style map; hist_s keeps the
    // smallest style count (the one style's count when there is one)
    int b = hs.h[0][l];
    bool ok = a > 10;
#pragma unroll
    for (int i = 0; i < CWCT_MAX_STYLES; ++i) {
        if (i < hs.n) {
            const int bi = hs.h[i][l];
            ok = ok && bi > 10 && (double)a / (double)bi < 100.0 && (double)bi / (double)a < 100.0;
            b = bi < b ? bi : b;
        }
    }
    valid[l] = ok;
    __syncthreads();
    if (l == 0) {
        int n = 0, over = 0;
        for (int k = 0; k < 256; ++k) {
            unsigned char s = 255;
            if (valid[k]) {
                if (n < cap) { s = (unsigned char)n; plan->slot_label[n] = (unsigned char)k; ++n; }
                else over = 1;
            }
            slot_of[k] = s;
        }
        for (int k = n; k < CWCT_MAX_SLOTS; ++k) plan->slot_label[k] = 0;
        plan->n_slots = n; plan->overflow = over;
        if (over && flags) atomicOr(flags, VST_MASK_OVERFLOW);
    }
    __syncthreads();
    plan->lut[l] = slot_of[to];
    plan->hist_c[l] = a;
    plan->hist_s[l] = b;
}

unsigned grid_for(long n, long per_thread) {
    long b = (n + 256 * per_thread - 1) / (256 * per_thread);
    return (unsigned)(b > 2048 ? 2048 : (b < 1 ? 1 : b));
}

}  // namespace

int vst_colors_to_labels(const uint8_t* rgb, uint8_t* labels, long n, void* stream) {
    if (!rgb || !labels || n <= 0) return VST_E_ARG;
    colors_to_labels_kernel<<<grid_for(n, 4), 256, 0, (hipStream_t)stream>>>(rgb, labels, n);
    VST_RETURN_IF_LAUNCH_FAILED();
    return VST_OK;
}

int vst_label_hist(const uint8_t* labels, long n, int* hist, void* stream) {
    if (!labels || !hist || n <= 0) return VST_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(hist, 0, 256 * sizeof(int), st);
    if (e != hipSuccess) return (int)e;
    hist_kernel<<<grid_for(n, 16), 256, 0, st>>>(labels, n, hist);
    VST_RETURN_IF_LAUNCH_FAILED();
    return VST_OK;
}

int vst_mask_prepare(const uint8_t* src, int colours, int H, int W, uint8_t* mask_rows, int* hist, void* stream) {
    if (!src || !mask_rows || !hist) return VST_E_ARG;
    if (!vst_shape_ok(1, H, W)) return VST_E_SHAPE;
    if ((((size_t)src) & 3) || (((size_t)mask_rows) & 7)) return VST_E_ARG;      // dword loads, 8-byte stores
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(hist, 0, 256 * sizeof(int), st);
    if (e != hipSuccess) return (int)e;
    const int Hq = H >> 2, Wq = W >> 2;
    const long pairs = ((long)Hq * Wq + 1) >> 1;
    const unsigned blocks = (unsigned)((2 * pairs + 255) / 256);
    if (colours) mask_prepare_kernel<true><<<blocks, 256, 0, st>>>(src, mask_rows, hist, Hq, Wq);
    else mask_prepare_kernel<false><<<blocks, 256, 0, st>>>(src, mask_rows, hist, Hq, Wq);
    VST_RETURN_IF_LAUNCH_FAILED();
    return VST_OK;
}

int vst_remap_lut(const int* hist, const int* style_hist, const int16_t* table, int rows, int cols, int min_count, uint8_t* lut,
                  int* hist_out, unsigned* flags, void* stream) {
    if (!hist || !table || !lut || min_count < 0) return VST_E_ARG;
    if (rows <= 0 || cols <= 0) return VST_E_SHAPE;
    remap_lut_kernel<<<1, 256, 0, (hipStream_t)stream>>>(hist, style_hist, table, rows, cols, min_count, lut, hist_out, flags);
    VST_RETURN_IF_LAUNCH_FAILED();
    return VST_OK;
}

int vst_apply_lut(const uint8_t* in, const uint8_t* lut, uint8_t* out, long n, void* stream) {
    if (!in || !lut || !out || n <= 0) return VST_E_ARG;
    apply_lut_kernel<<<grid_for(n, 4), 256, 0, (hipStream_t)stream>>>(in, lut, out, n);
    VST_RETURN_IF_LAUNCH_FAILED();
    return VST_OK;
}

int vst_label_plan_hist(const int* hist_c, const uint8_t* remap_lut, const int* hist_s, int max_slots, void* plan,
                        unsigned* flags, void* stream) {
    if (!hist_c || !hist_s || !plan) return VST_E_ARG;
    if (max_slots < 1 || max_slots > CWCT_MAX_SLOTS) return VST_E_SHAPE;
    StyleHists hs{};
    hs.h[0] = hist_s; hs.n = 1;
    label_plan_hist_kernel<<<1, 256, 0, (hipStream_t)stream>>>(hist_c, remap_lut, hs, max_slots, (LabelPlan*)plan, flags);
    VST_RETURN_IF_LAUNCH_FAILED();
    return VST_OK;
}

int vst_label_plan_hists(const int* hist_c, const uint8_t* remap_lut, const int* const* hist_s_host_array, int n_styles,
                         int max_slots, void* plan, unsigned* flags, void* stream) {
    if (!hist_c || !hist_s_host_array || !plan) return VST_E_ARG;
    if (n_styles < 1 || n_styles > CWCT_MAX_STYLES) return VST_E_ARG;
    if (max_slots < 1 || max_slots > CWCT_MAX_SLOTS) return VST_E_SHAPE;
    StyleHists hs{};
    for (int i = 0; i < n_styles; ++i) {
        if (!hist_s_host_array[i]) return VST_E_ARG;
        hs.h[i] = hist_s_host_array[i];
    }
    hs.n = n_styles;
    label_plan_hist_kernel<<<1, 256, 0, (hipStream_t)stream>>>(hist_c, remap_lut, hs, max_slots, (LabelPlan*)plan, flags);
    VST_RETURN_IF_LAUNCH_FAILED();
    return VST_OK;
}
