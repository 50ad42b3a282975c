// Temporal stabiliser (vstnet.h, "Stabiliser"; DESIGN.md section 6, "Stabiliser"): the frame that is about to be written, blended
// with the previously written frame sampled along the flow, where the INPUT did not change along that flow.
//
// One thread per pixel, no atomics, no workspace.  All arithmetic is fp64 without contraction and uses only + - * /, comparisons
// and rint, each correctly rounded, so the device is held to a numpy statement of the same formula (tests/stabilise_ref.py) byte
// for byte.  A pixel that is not live - its sample position outside the frame or not finite, or masked out - copies cur_out and
// never forms an index from that position.
#include "common.h"
#include <math.h>

#pragma clang fp contract(off)

namespace {

__device__ __forceinline__ int clampi(int v, int n) { return v < 0 ? 0 : (v > n - 1 ? n - 1 : v); }

__global__ __launch_bounds__(256) void stabilise_kernel(const uint8_t* __restrict__ cur_in, const uint8_t* __restrict__ prev_in,
                                                        const uint8_t* __restrict__ cur_out, const uint8_t* __restrict__ prev_written,
                                                        const float* __restrict__ flow, const uint8_t* __restrict__ valid,
                                                        uint8_t* __restrict__ written, int h, int w, double gain, double sigma,
                                                        double limit) {
    const size_t hw = (size_t)h * w;
    const size_t at = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (at >= hw) return;
    const int y = (int)(at / w), x = (int)(at % w);
    const double qx = (double)x - (double)flow[at], qy = (double)y - (double)flow[hw + at];
    const bool inside = qx >= 0.0 && qx <= (double)(w - 1) && qy >= 0.0 && qy <= (double)(h - 1);     // false for NaN, +-inf
    const bool live = inside && (valid == nullptr || valid[at] != 0);
    const double s[3] = {(double)cur_out[at * 3], (double)cur_out[at * 3 + 1], (double)cur_out[at * 3 + 2]};
    if (!live) {
#pragma unroll
        for (int c = 0; c < 3; ++c) written[at * 3 + c] = cur_out[at * 3 + c];
        return;
    }
    // consistency_kernel's sample (flow.hip): q is inside, the clamps and clampi are the same statements
    const double cx = fmin(fmax(qx, 0.0), (double)(w - 1)), cy = fmin(fmax(qy, 0.0), (double)(h - 1));
    const int x0 = clampi((int)floor(cx), w), y0 = clampi((int)floor(cy), h);
    const int x1 = x0 + 1 > w - 1 ? w - 1 : x0 + 1, y1 = y0 + 1 > h - 1 ? h - 1 : y0 + 1;
    const double ax = cx - (double)x0, ay = cy - (double)y0;
    const size_t p00 = ((size_t)y0 * w + x0) * 3, p01 = ((size_t)y0 * w + x1) * 3;
    const size_t p10 = ((size_t)y1 * w + x0) * 3, p11 = ((size_t)y1 * w + x1) * 3;
    double d[3], o[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double itop = (1.0 - ax) * (double)prev_in[p00 + c] + ax * (double)prev_in[p01 + c];
        const double ibot = (1.0 - ax) * (double)prev_in[p10 + c] + ax * (double)prev_in[p11 + c];
        d[c] = (double)cur_in[at * 3 + c] - ((1.0 - ay) * itop + ay * ibot);
        const double otop = (1.0 - ax) * (double)prev_written[p00 + c] + ax * (double)prev_written[p01 + c];
        const double obot = (1.0 - ax) * (double)prev_written[p10 + c] + ax * (double)prev_written[p11 + c];
        o[c] = (1.0 - ay) * otop + ay * obot;
    }
    const double e = ((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) / 3.0;
    const double wgt = gain / (1.0 + e / (sigma * sigma));
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double delta = fmin(fmax(wgt * (o[c] - s[c]), -limit), limit);
        written[at * 3 + c] = (uint8_t)fmin(fmax(rint(s[c] + delta), 0.0), 255.0);
    }
}

bool off_grid(const void* p, uintptr_t bytes) { return (((uintptr_t)p) & (bytes - 1)) != 0; }

bool overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return a && b && pa < pb + nb && pb < pa + na;
}

}  // namespace

int vst_stabilise_u8(const uint8_t* cur_in, const uint8_t* prev_in, const uint8_t* cur_out, const uint8_t* prev_written,
                     const float* flow, const uint8_t* valid_or_null, int h, int w, double gain, double sigma, double limit,
                     uint8_t* written, void* stream) {
    if (!cur_in || !prev_in || !cur_out || !prev_written || !flow || !written) return VST_E_ARG;
    if (h < 1 || w < 1 || (int64_t)h * w > VST_MAX_FRAME_PIXELS) return VST_E_SHAPE;
    if (!(gain > 0.0 && gain < 1.0) || !(sigma > 0.0 && sigma < INFINITY) || !(limit >= 0.0 && limit < INFINITY)) return VST_E_ARG;
    const size_t n = (size_t)h * w;
    if (off_grid(flow, 4)) return VST_E_ARG;
    // the blend gathers from the previous pair, and cur_out is the frame the caller goes on to compare with: never in place
    if (overlap(written, n * 3, prev_written, n * 3) || overlap(written, n * 3, cur_out, n * 3) ||
        overlap(written, n * 3, prev_in, n * 3) || overlap(written, n * 3, cur_in, n * 3) || overlap(written, n * 3, flow, n * 8) ||
        overlap(written, n * 3, valid_or_null, n))
        return VST_E_ARG;
    stabilise_kernel<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream>>>(cur_in, prev_in, cur_out, prev_written, flow,
                                                                                   valid_or_null, written, h, w, gain, sigma, limit);
    VST_RETURN_IF_LAUNCH_FAILED();
    return VST_OK;
}
